#!/usr/bin/env python3
"""Throughput of the engine-backed task module against the raw engine it replays: AV-MNIST M2-Mixer-B, bf16, dropout 0.5,
batch 512.  Both in one process over the same device-resident batches, after warm-up, timed with HIP events, in alternating
repetitions:
  engine_replay   the raw engine's captured step (engine.capture -> replay(batch)), the INTEGRATION.md section 2 low-level loop;
  bound_module    AVMnistMixerMultiLoss after bind_engine(512): training_step(batch) -- the same replay plus the cloned
                  losses / predictions and the host-side learning-rate check.
Prints one JSON line: samples/s of each (best repetition) and bound / raw.
Usage: python scripts/engine_backed_throughput.py [--steps 200] [--warmup 20] [--reps 3] [--batches 8]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                   # noqa: E402  (configs and the synthetic batch generator only)
import m2_mixer_amd as M                       # noqa: E402
from m2_mixer_amd import models as MD          # noqa: E402


def make_net(cfg, B, dev):
    M.set_precision("bf16")
    mods = {"image": dict(cfg["image"], block_type="MLPMixer"), "audio": dict(cfg["audio"], block_type="MLPMixer"),
            "multimodal": dict(cfg["multimodal"], block_type="FusionMixer", fusion_function="ConcatFusion"),
            "classification": dict(classifier="StandardClassifier", num_classes=cfg["num_classes"],
                                   input_shape=[B, bench.n_patch(cfg["image"]) + bench.n_patch(cfg["audio"]), cfg["multimodal"]["hidden_dim"]])}
    torch.manual_seed(42)
    return MD.AVMnistMixerMultiLoss({"dropout": cfg["dropout"], "modalities": mods},
                                    {"lr": 1e-3, "betas": (0.9, 0.999), "scheduler_patience": 2}).to(dev)


def timed(step, batches, n):
    """ms per step over n steps (HIP events around the enqueue of the whole loop)."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(n):
        step(batches[i % len(batches)])
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg, B = dict(bench.CFG_B, dropout=0.5), 512
    batches = []
    for i in range(args.batches):
        image, audio, labels = bench.make_batch(cfg, B, 1234 + i, dev)
        batches.append({"image": image, "audio": audio, "label": labels})

    raw_net = make_net(cfg, B, dev)
    eng = raw_net.to_engine(B, precision="bf16")
    b0 = batches[0]
    replay = eng.capture(b0["image"], b0["audio"], b0["label"])
    raw_step = lambda b: replay(b["image"], b["audio"], b["label"])

    net = make_net(cfg, B, dev)
    net.bind_engine(B, precision="bf16")
    net.configure_optimizers()                   # the lr check of every training_step is part of what is timed
    bound_step = lambda b: net.training_step(b, 0)

    for fn in (raw_step, bound_step):
        timed(fn, batches, args.warmup)          # (the bound module captures its graph on its first step)
    raw_ms, bound_ms = [], []
    for _ in range(args.reps):
        raw_ms.append(timed(raw_step, batches, args.steps))
        bound_ms.append(timed(bound_step, batches, args.steps))
    raw, bound = B / (min(raw_ms) * 1e-3), B / (min(bound_ms) * 1e-3)
    print(json.dumps({"workload": "avmnist_m2-mixer_B bf16 dropout 0.5", "batch": B, "steps": args.steps, "reps": args.reps,
                      "engine_replay_samples_per_s": round(raw, 1), "bound_module_samples_per_s": round(bound, 1),
                      "ratio": round(bound / raw, 4), "engine_replay_ms": [round(x, 4) for x in raw_ms],
                      "bound_module_ms": [round(x, 4) for x in bound_ms], "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
