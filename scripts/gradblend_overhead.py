#!/usr/bin/env python3
"""What one Gradient-Blending refresh costs on the fused engines: one JSON line per shape.

  refresh   gradblend.GradBlend(engine, split).get_weights(), host wall clock around the call with a device synchronisation on
            both sides (it builds two clones and their siblings, captures two graphs, trains 2 x epochs passes and probes six):
            --reps repetitions after one untimed call, median and spread (max - min);
  training  the same number of ORDINARY captured training steps (3 x epochs x batches: what the reference's three retrainings
            run), HIP events around the replays -- the work a refresh would cost if each of its models were a full step.

Shapes: M2-Mixer-B at batch 512, MIMIC-H at 128 (bf16), --batches batches in the split (a tenth of them, at least one, are val).
Usage: python scripts/gradblend_overhead.py [--epochs 20] [--batches 20] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feed_overhead import events, synthetic_split          # noqa: E402
from scores_overhead import CASES, E                      # noqa: E402
from m2_mixer_amd.data import ResidentTensors              # noqa: E402
from m2_mixer_amd.gradblend import GradBlend               # noqa: E402


def measure(name, cls, c, mk, B, dev, args):
    eng = getattr(E, cls)(c, B, device=dev, precision="bf16", lr=1e-3)
    split = synthetic_split(mk, c, B, args.batches, dev)
    data = ResidentTensors({"train": split})
    nval = max(1, args.batches // 10)
    gb = GradBlend(eng, data, val_fraction=(nval * B + 0.5) / (args.batches * B), epochs=args.epochs)
    gb.get_weights()                                      # untimed: lazy initialisation of every launch form
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ws = gb.get_weights()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    steps = 3 * args.epochs * (args.batches - nval)
    batch = tuple(t[:B].contiguous() for t in split)
    replay = eng.clone().capture(*batch)
    events(lambda i: replay(), 20)
    ordinary = events(lambda i: replay(), steps) * steps * 1e-3      # events(): ms per step
    return {"measure": "refresh", "case": name, "batch": B, "precision": "bf16", "epochs": args.epochs, "train_batches": args.batches - nval,
            "val_batches": nval, "reps": args.reps, "refresh_s": round(statistics.median(times), 4),
            "refresh_spread_s": round(max(times) - min(times), 4), "refresh_reps_s": [round(t, 4) for t in times],
            "ordinary_steps": steps, "ordinary_steps_s": round(ordinary, 4), "weights": {k: round(v, 6) for k, v in ws.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, cls, c, mk, B in CASES[:2]:
        row = measure(name, cls, c, mk, B, dev, args)
        row.update(device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
