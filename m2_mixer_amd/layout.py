"""Parameter layout of the fused engines (engine.py): state-dict key -> shape in the reference's creation order for every
model, the fusion function's name and token count, and the flat ranges a training stage trains.  Pure functions of a cfg dict:
no device, no library call (from runtime only the MixerBlock key and shape tables are taken), so host code and host tests
can lay a model out without the engines.  engine.py re-exports every name here.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

from .runtime import BLOCK_FIELDS, BLOCK_KEYS, block_param_shapes


def _num_patch(c: dict) -> int:
    return (c["image_size"][0] // c["patch_size"]) * (c["image_size"][1] // c["patch_size"])


def _tower_shapes(s: "OrderedDict[str, tuple]", prefix: str, c: dict, N: int, embed: Optional[str]):
    D = c["hidden_dim"]
    if embed == "patch":
        s[prefix + "to_patch_embedding.0.weight"] = (D, c["in_channels"], c["patch_size"], c["patch_size"])
        s[prefix + "to_patch_embedding.0.bias"] = (D,)
    elif embed == "proj":
        s[prefix + "proj.weight"] = (c["proj_dim"], c["embedding_dim"])
        s[prefix + "proj.bias"] = (c["proj_dim"],)
    shapes = block_param_shapes(D, N, c["token_dim"], c["channel_dim"])
    for i in range(c["num_mixers"]):
        for f in BLOCK_FIELDS:
            s[f"{prefix}mixer_blocks.{i}.{BLOCK_KEYS[f]}"] = shapes[f]
    s[prefix + "layer_norm.weight"] = (D,)
    s[prefix + "layer_norm.bias"] = (D,)


def _head_shapes(s, names: Sequence[str], dims: Sequence[int], K: int):
    for n, d in zip(names, dims):
        key = "classifier_fusion.classifer." if n == "fusion" else f"classifier_{n}."     # sic: classification.py:87
        s[key + "weight"] = (K, d)
        s[key + "bias"] = (K,)


#: fusion functions (cfg["multimodal"]["fusion_function"]) the two-tower engines build; ConcatFusion when the key is absent
ENGINE_FUSIONS = ("ConcatFusion", "SumFusion", "MeanFusion", "MaxFusion", "BiModalGatedUnit")


def fusion_function_name(mm: dict) -> str:
    """cfg["multimodal"]'s fusion function; refuses the ones the engines do not build (ConcatDynaFusion, ExtraConcatFusion)."""
    name = mm.get("fusion_function", "ConcatFusion")
    if name not in ENGINE_FUSIONS:
        raise RuntimeError(f"multimodal.fusion_function = {name!r}: the fused engines build {', '.join(ENGINE_FUSIONS)}")
    return name


def fusion_tokens(mm: dict, na: int, nb: int) -> int:
    """Tokens of the fusion tower: the registry's own get_output_shape(na, nb, dim=1) (models/avmnist.py:183-186), so unequal
    token counts are refused as the reference refuses them (sum / mean / max: ValueError)."""
    from .modules import fusion as F
    name = fusion_function_name(mm)
    if name == "BiModalGatedUnit":
        if na != nb:       # (its get_output_shape does not check; the reference fails inside torch.cat)
            raise RuntimeError(f"multimodal.fusion_function = BiModalGatedUnit needs equal token counts, got {na} and {nb}")
        return na
    fn = F.ConcatFusion(dim=1) if name == "ConcatFusion" else getattr(F, name)()
    return int(fn.get_output_shape(na, nb, dim=1))


def two_tower_param_shapes(cfg: dict, mods: Tuple[str, str]) -> "OrderedDict[str, tuple]":
    """state-dict key -> shape in the reference's creation order (models/avmnist.py:181-191, models/mmimdb.py:35-45): the two
    towers, the fusion function's parameters (BiModalGatedUnit only), the fusion mixer, the three heads."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    a, b = mods
    mm = cfg["multimodal"]
    na, nb = _num_patch(cfg[a]), _num_patch(cfg[b])
    nf = fusion_tokens(mm, na, nb)
    _tower_shapes(s, f"{a}_mixer.", cfg[a], na, "patch")
    _tower_shapes(s, f"{b}_mixer.", cfg[b], nb, "patch")
    if fusion_function_name(mm) == "BiModalGatedUnit":
        i1, i2, o = mm["mod1_in"], mm["mod2_in"], mm["out_size"]
        for k, fan_in in (("mod1_hidden", i1), ("mod2_hidden", i2), ("z_hidden", i1 + i2)):       # modules/fusion.py:10-14
            s[f"fusion_function.{k}.weight"] = (o, fan_in)
            s[f"fusion_function.{k}.bias"] = (o,)
    _tower_shapes(s, "fusion_mixer.", mm, nf, None)
    _head_shapes(s, (a, b, "fusion"), (cfg[a]["hidden_dim"], cfg[b]["hidden_dim"], cfg["multimodal"]["hidden_dim"]),
                 cfg["num_classes"])
    return s


def avmnist_param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    return two_tower_param_shapes(cfg, ("image", "audio"))


def mimic_param_shapes(cfg: dict) -> "OrderedDict[str, tuple]":
    """Creation order of models/mimic.py:39-49: time_mixer, static_extractor, fusion_mixer, three classifiers."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    t, st = cfg["time"], cfg["static"]
    _tower_shapes(s, "time_mixer.", t, t["num_patch"], "proj")
    for i in range(st["num_blocks"]):
        s[f"static_extractor.module_list.{3 * i}.weight"] = (st["hidden_dim"], st["input_dim"] if i == 0 else st["hidden_dim"])
        s[f"static_extractor.module_list.{3 * i}.bias"] = (st["hidden_dim"],)
    k = 3 * st["num_blocks"]
    s[f"static_extractor.module_list.{k}.weight"] = (st["output_dim"], st["hidden_dim"])
    s[f"static_extractor.module_list.{k}.bias"] = (st["output_dim"],)
    _tower_shapes(s, "fusion_mixer.", cfg["multimodal"], 1 + t["num_patch"], None)
    _head_shapes(s, ("static", "time", "fusion"), (st["output_dim"], t["hidden_dim"], cfg["multimodal"]["hidden_dim"]),
                 cfg["num_classes"])
    return s


def trainable_flat_ranges(shapes: "Dict[str, tuple]", frozen_prefixes: Sequence[str], invert: bool = False) -> List[Tuple[int, int]]:
    """Stage two of the reference's two-stage training (models/avmnist.py:314-324): the contiguous flat ranges [lo, hi) of the
    parameters that keep training, given the ordered state-dict shapes and the key prefixes that freeze.  Neighbouring trainable
    parameters are merged; the ranges are sorted and disjoint, and with the frozen keys' ranges they tile [0, n_params).  Pure:
    no device, no library.
    invert=True: the complement -- the ranges of the keys that DO start with one of the prefixes (the modalities-only stage
    trains exactly what stage two freezes: train_modalities_only)."""
    frozen = tuple(frozen_prefixes)
    out: List[Tuple[int, int]] = []
    off = 0
    for k, shp in shapes.items():
        cnt = 1
        for d in shp:
            cnt *= int(d)
        if k.startswith(frozen) == invert:
            if out and out[-1][1] == off:
                out[-1] = (out[-1][0], off + cnt)
            else:
                out.append((off, off + cnt))
        off += cnt
    return out


def frozen_key_prefixes(names: Sequence[str]) -> Tuple[str, ...]:
    """Key prefixes that stage two freezes for the modalities `names` (_MultiLossModule._freeze_modalities): the two modality
    towers with their embeddings (MIMIC: static_extractor, time_mixer) and their two heads."""
    towers = ("static_extractor.", "time_mixer.") if tuple(names) == ("static", "time") else tuple(f"{n}_mixer." for n in names)
    return towers + tuple(f"classifier_{n}." for n in names)


def _is_layer_norm(k: str) -> bool:
    return ("layer_norm." in k) or k.endswith("token_mix.0.weight") or k.endswith("token_mix.0.bias") \
        or k.endswith("channel_mix.0.weight") or k.endswith("channel_mix.0.bias")
