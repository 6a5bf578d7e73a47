#!/usr/bin/env python3
"""Captured training-step time of the fused engines for each fusion function: one JSON line per (shapes, fusion, batch) with
the replayed step's ms (HIP events around --steps replays after --warmup, best of --reps), its ratio to ConcatFusion at the
same shapes and batch, and the same model on the graphed module path (graphs.GraphedStep over the task module with torch
autograd + fused Adam) for comparison.  bf16, dropout as in the cfg.  Cases: M2-Mixer-B at batch 512; the gated_4loss shapes (49-token towers)
at 512 and at its cfg batch 32; MM-IMDb at its cfg batch 32.
Usage: python scripts/fusion_configs.py [--steps 200] [--warmup 20] [--reps 3] [--only SHAPES:FUSION:BATCH]
(--only: that one case, e.g. gated_4loss:BiModalGatedUnit:512 under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import fusion_ref as R                         # noqa: E402  (the gated_4loss shapes, with_fusion)
import gen_util as G                           # noqa: E402
from m2_mixer_amd.engine import AVMnistEngine, MMIMDBEngine  # noqa: E402

FUSIONS = ("ConcatFusion", "SumFusion", "MeanFusion", "MaxFusion", "BiModalGatedUnit")
CASES = [("avmnist_B", "avmnist", G.AVMNIST["B"], 512), ("gated_4loss", "avmnist", R.GATED_4LOSS, 512),
         ("gated_4loss", "avmnist", R.GATED_4LOSS, 32), ("mmimdb", "mmimdb", G.MMIMDB, 32)]


def step_ms(task, c, B, dev, args):
    cls = AVMnistEngine if task == "avmnist" else MMIMDBEngine
    eng = cls(c, B, device=dev, precision="bf16", lr=1e-3)
    mk = G.avmnist_batch if task == "avmnist" else G.mmimdb_batch
    batches = [[t.to(dev) for t in mk(B, 100 + i, c)] for i in range(4)]
    replay = eng.capture(*batches[0])
    for i in range(args.warmup):
        replay(*batches[i % 4])
    best = []
    for _ in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(args.steps):
            replay(*batches[i % 4])
        e.record()
        e.synchronize()
        best.append(s.elapsed_time(e) / args.steps)
    return min(best), best


def module_ms(task, c, B, dev, args):
    """The same model as a task module (modules/ + torch autograd), one GraphedStep replay per step."""
    import m2_mixer_amd as M
    from m2_mixer_amd import models as MD
    from m2_mixer_amd.graphs import GraphedStep
    M.set_precision("bf16")
    a, b = ("image", "audio") if task == "avmnist" else ("image", "text")
    mods = {a: dict(c[a], block_type="MLPMixer"), b: dict(c[b], block_type="MLPMixer"),
            "multimodal": dict(c["multimodal"], block_type="FusionMixer"),
            "classification": dict(classifier="StandardClassifier", num_classes=c["num_classes"],
                                              input_shape=[B, 1, c["multimodal"]["hidden_dim"]])}
    cfg = {"dropout": c["dropout"], "modalities": mods}
    if task == "mmimdb":
        cfg["pos_weight"] = c["pos_weight"]
    cls = MD.AVMnistMixerMultiLoss if task == "avmnist" else MD.MMIMDBMixerMultiLoss
    torch.manual_seed(42)
    net = cls(cfg, {"lr": 1e-3, "betas": (0.9, 0.999), "scheduler_patience": 2}).to(dev)
    net.train()
    opt = net.configure_optimizers()["optimizer"]
    mk = G.avmnist_batch if task == "avmnist" else G.mmimdb_batch
    xa, xb, y = [t.to(dev) for t in mk(B, 100, c)]
    batch = {a: xa, b: xb, "label": y}
    step = GraphedStep(net, opt, batch)
    for _ in range(args.warmup):
        step(batch)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(50, args.steps // 4)
    s.record()
    for _ in range(n):
        step(batch)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-module", dest="module", action="store_false", help="skip the graphed module path")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shapes, task, base, B in CASES:
        concat = None
        for fusion in FUSIONS:
            if shapes == "mmimdb" and fusion in ("MeanFusion", "MaxFusion"):
                continue
            if args.only and args.only != f"{shapes}:{fusion}:{B}":
                continue
            ms, reps = step_ms(task, R.with_fusion(base, fusion), B, dev, args)
            concat = ms if fusion == "ConcatFusion" else concat
            mod = round(module_ms(task, R.with_fusion(base, fusion), B, dev, args), 4) if args.module else None
            print(json.dumps({"module_path_graphed_ms": mod, "engine_speedup_vs_module": round(mod / ms, 3) if mod else None,"shapes": shapes, "fusion": fusion, "batch": B, "precision": "bf16", "step_ms": round(ms, 4),
                              "reps_ms": [round(x, 4) for x in reps], "vs_concat": round(ms / concat, 4) if concat else None,
                              "samples_per_s": round(B / (ms * 1e-3), 1), "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
