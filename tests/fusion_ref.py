"""Float64 restatement of the fusion functions the fused engines build (the reference's modules/fusion.py:7-55, :190-221,
:258-272) and of the AV-MNIST / MM-IMDb training step with the fusion in place of concat_fusion, out of the oracle's
primitives (models/avmnist.py:259-298, models/mmimdb.py:96-147)."""
from collections import OrderedDict

import torch

from oracle import m2mixer_oracle as O

FUSIONS = ("SumFusion", "MeanFusion", "MaxFusion", "BiModalGatedUnit")
GATE_KEYS = ("mod1_hidden", "mod2_hidden", "z_hidden")

# gated_4loss: cfg/avmnist/avmnist_gated_4loss.yml (49-token towers, D = 128)
GATED_4LOSS = dict(dropout=0.5, num_classes=10,
                   image=dict(in_channels=1, hidden_dim=128, patch_size=4, image_size=[28, 28], token_dim=32, channel_dim=3072, num_mixers=4),
                   audio=dict(in_channels=1, hidden_dim=128, patch_size=16, image_size=[112, 112], token_dim=32, channel_dim=3072, num_mixers=4),
                   multimodal=dict(hidden_dim=128, token_dim=32, channel_dim=3072, num_mixers=2))


def with_fusion(c: dict, name: str) -> dict:
    """The task config `c` with multimodal.fusion_function = name (the gate's sizes: the towers' hidden_dim)."""
    mm = dict(c["multimodal"], fusion_function=name)
    if name == "BiModalGatedUnit":
        D = mm["hidden_dim"]
        mm.update(mod1_in=D, mod2_in=D, out_size=D)
    return dict(c, multimodal=mm)


def gate_shapes(mm: dict) -> "OrderedDict[str, tuple]":
    i1, i2, o = mm["mod1_in"], mm["mod2_in"], mm["out_size"]
    s = OrderedDict()
    for k, fi in zip(GATE_KEYS, (i1, i2, i1 + i2)):
        s[f"fusion_function.{k}.weight"] = (o, fi)
        s[f"fusion_function.{k}.bias"] = (o,)
    return s


def gate(a, b, p, prefix="fusion_function."):
    """BiModalGatedUnit.forward: z * tanh(W1 a + b1) + (1 - z) * tanh(W2 b + b2), z = sigmoid(Wz [a, b] + bz)."""
    h1 = torch.tanh(O.linear(a, p[prefix + "mod1_hidden.weight"], p[prefix + "mod1_hidden.bias"]))
    h2 = torch.tanh(O.linear(b, p[prefix + "mod2_hidden.weight"], p[prefix + "mod2_hidden.bias"]))
    z = torch.sigmoid(O.linear(torch.cat([a, b], dim=-1), p[prefix + "z_hidden.weight"], p[prefix + "z_hidden.bias"]))
    return z * h1 + (1 - z) * h2


def fuse(name: str, a, b, p=None):
    if name == "ConcatFusion":
        return O.concat_fusion(a, b, dim=1)
    if name == "SumFusion":
        return torch.add(a, b)
    if name == "MeanFusion":
        return torch.stack([a, b]).mean(0)
    if name == "MaxFusion":
        return torch.maximum(a, b)
    if name == "BiModalGatedUnit":
        return gate(a, b, p)
    raise ValueError(name)


def two_tower_shapes(task: str, c: dict) -> "OrderedDict[str, tuple]":
    """The oracle's parameter shapes with the gate's keys between the second tower and `fusion_mixer.`, and the fusion mixer
    sized for the fusion's token count."""
    import gen_util as G
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    mm = c["multimodal"]
    name = mm.get("fusion_function", "ConcatFusion")
    na, nb = G.num_patch(c[a]), G.num_patch(c[b])
    nf = na + nb if name == "ConcatFusion" else na
    s = OrderedDict()
    s.update(G.tower_shapes(f"{a}_mixer.", c[a], na, "patch"))
    s.update(G.tower_shapes(f"{b}_mixer.", c[b], nb, "patch"))
    if name == "BiModalGatedUnit":
        s.update(gate_shapes(mm))
    s.update(G.tower_shapes("fusion_mixer.", mm, nf, "none"))
    K = c["num_classes"]
    for n in (a, b):
        s[f"classifier_{n}.weight"] = (K, c[n]["hidden_dim"])
        s[f"classifier_{n}.bias"] = (K,)
    s["classifier_fusion.classifer.weight"] = (K, mm["hidden_dim"])
    s["classifier_fusion.classifer.bias"] = (K,)
    return s


def two_tower_forward(task: str, xa, xb, labels, p, c: dict, pos_weight=None, fusion_loss_weight: float = 1.0 / 3):
    """shared_step of AVMnistMixerMultiLoss / MMIMDBMixerMultiLoss (dropout off) with c["multimodal"]["fusion_function"]."""
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    name = c["multimodal"].get("fusion_function", "ConcatFusion")
    ta = O.mlp_mixer(xa, p, f"{a}_mixer.", c[a]["patch_size"], c[a]["num_mixers"])
    tb = O.mlp_mixer(xb, p, f"{b}_mixer.", c[b]["patch_size"], c[b]["num_mixers"])
    ft = O.fusion_mixer(fuse(name, ta, tb, p), p, "fusion_mixer.", c["multimodal"]["num_mixers"])
    la = O.linear(ta.mean(1), p[f"classifier_{a}.weight"], p[f"classifier_{a}.bias"])
    lb = O.linear(tb.mean(1), p[f"classifier_{b}.weight"], p[f"classifier_{b}.bias"])
    lf = O.standard_classifier(ft, p["classifier_fusion.classifer.weight"], p["classifier_fusion.classifer.bias"])
    if task == "avmnist":
        l_a, l_b, l_f = O.cross_entropy(la, labels), O.cross_entropy(lb, labels), O.cross_entropy(lf, labels)
        ow = (1 - fusion_loss_weight) / 2
        loss = (fusion_loss_weight * l_f + ow * l_a + ow * l_b) * 3
        preds = torch.softmax(lf, dim=1).argmax(dim=1)
    else:
        y = labels.to(lf.dtype)
        pw = pos_weight.to(lf.dtype)
        l_a, l_b, l_f = O.bce_with_logits(la, y, pw), O.bce_with_logits(lb, y, pw), O.bce_with_logits(lf, y, pw)
        loss = l_a + l_b + l_f
        preds = (torch.sigmoid(lf) > 0.5).long()
    return {"logits": torch.stack([la, lb, lf]), "losses": torch.stack([l_a, l_b, l_f, loss]), "loss": loss, "preds": preds}


class Step:
    """Autograd through two_tower_forward in float64, then torch.optim.Adam's update (oracle.adam_step) of every parameter."""

    def __init__(self, task, c, params, lr, pos_weight=None):
        self.task, self.c, self.lr, self.pw = task, c, lr, pos_weight
        self.p = {k: v.detach().double().clone() for k, v in params.items()}
        self.t, self.m, self.v = 0, {}, {}

    def forward(self, xa, xb, labels):
        with torch.no_grad():
            return two_tower_forward(self.task, xa.double(), xb.double(), labels, self.p, self.c, self.pw)

    def step(self, xa, xb, labels):
        leaves = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        out = two_tower_forward(self.task, xa.double(), xb.double(), labels, leaves, self.c, self.pw)
        out["loss"].backward()
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
