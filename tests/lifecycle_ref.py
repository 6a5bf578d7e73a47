"""The float64 side of the module-path lifecycle tests (tests/lifecycle_cases.py): for each model of the table its state-dict
shapes, seeded batches and the oracle's forward, shared by tests/test_gpu_module_lifecycle.py (the reference every observation is
held to) and tests/test_host_lifecycle.py (the condition on learning rate and seeds, checked without a GPU)."""
import torch

import gen_util as G
from lifecycle_cases import MODELS, is_packed
from oracle import m2mixer_oracle as O

HEADS = {"avmnist": ("logits", "image_logits", "audio_logits"), "mimic": ("logits", "logits_static", "logits_time"),
         "mmimdb": ("logits", "image_logits", "text_logits"), "deep": ("tokens",)}
# the heads a tower feeds: MIMIC's `logits_static` comes from the static MLP alone, which keeps no packed copy
TOWER_FED = {"avmnist": HEADS["avmnist"], "mimic": ("logits", "logits_time"), "mmimdb": HEADS["mmimdb"], "deep": ("tokens",)}


class Ref:
    def __init__(self, name):
        self.name, self.info = name, MODELS[name]
        self.B = self.info["B"]
        # the configs tests/test_gpu_parity.py::_model_cfg builds the task modules from (dropout is set to 0 there and here)
        self.c = {"avmnist": G.AVMNIST["S"], "mimic": G.MIMIC_H, "mmimdb": G.MMIMDB, "deep": self.info.get("cfg")}[name]
        self.shapes = {"avmnist": G.avmnist_shapes, "mimic": G.mimic_shapes, "mmimdb": G.mmimdb_shapes,
                       "deep": lambda c: G.tower_shapes("", c, self.info["N"], "none")}[name](self.c)

    def params(self, seed=None):
        return G.make_params(self.shapes, self.info["seed"] if seed is None else seed)

    def batch(self, seed):
        """A fresh CPU batch in the layout shared_step takes (deep: the tokens alone)."""
        if self.name == "avmnist":
            return dict(zip(("image", "audio", "label"), G.avmnist_batch(self.B, seed, self.c)))
        if self.name == "mmimdb":
            return dict(zip(("image", "text", "label"), G.mmimdb_batch(self.B, seed, self.c)))
        if self.name == "mimic":
            return G.mimic_batch(self.B, seed, self.c)
        return (torch.randn(self.B, self.info["N"], self.c["hidden_dim"], generator=torch.Generator().manual_seed(seed)),)

    def forward(self, batch, p):
        """The heads (HEADS) and the training loss from the float64 oracle at the parameters `p` (float64, CPU)."""
        d = lambda t: t.double() if torch.is_floating_point(t) else t
        if self.name == "deep":
            y = O.fusion_mixer(d(batch[0]), p, "", self.c["num_mixers"])
            return {"tokens": y, "loss": y.square().sum()}
        if self.name == "avmnist":
            out = O.avmnist_forward(d(batch["image"]), d(batch["audio"]), batch["label"], p, self.c)
        elif self.name == "mmimdb":
            out = O.mmimdb_forward(d(batch["image"]), d(batch["text"]), d(batch["label"]), p, self.c,
                                   torch.tensor(self.c["pos_weight"], dtype=torch.float64))
        else:
            out = O.mimic_forward(d(batch[0]), d(batch[1]), batch[2], p, self.c)
        return {k: out[k] for k in HEADS[self.name] + ("loss",)}

    def stale_distance(self, batch, cur, prev, true=None):
        """How far the logits move, in the head of TOWER_FED that moves least, when the packed tensors alone are taken from
        `prev` (the weights of before the last update) and everything else from `cur`."""
        with torch.no_grad():
            true = self.forward(batch, cur) if true is None else true
            old = self.forward(batch, {k: (prev[k] if is_packed(k) else v) for k, v in cur.items()})
            return min(float((old[k] - true[k]).abs().max()) for k in TOWER_FED[self.name])
