#!/usr/bin/env python3
"""What stage two of the two-stage training costs and returns: one JSON line per measurement.

  step    the captured training step in stage two (engine.freeze_modalities) beside the captured stage-one step, bf16: two engines
          of one configuration in ONE process, one of them frozen; HIP events around --steps replays after --warmup, --reps
          repetitions with the two INTERLEAVED repetition by repetition; medians and the spread (max - min) of each.
  gather  m2m_feed_gather_muted with code 0 (nothing muted), input a muted and input b muted beside m2m_feed_gather, filling one
          step's input slots from a shuffled resident split of 16 batches -- the method of scripts/feed_overhead.py.

Shapes: M2-Mixer-B at batch 512, MIMIC-H at 128, MM-IMDb at 32 (`gather`: M2-Mixer-B only).
Usage: python scripts/two_stage_overhead.py [--steps 200] [--warmup 20] [--reps 5] [--only step|gather] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from feed_overhead import events, synthetic_split          # noqa: E402
from scores_overhead import CASES, E                      # noqa: E402


def summary(times):
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {**{k + "_us": round(v * 1e3, 2) for k, v in med.items()},
                 **{k + "_spread_us": round((max(v) - min(v)) * 1e3, 2) for k, v in times.items()},
                 **{k + "_reps_us": [round(x * 1e3, 2) for x in v] for k, v in times.items()}}


def measure_step(name, cls, c, mk, B, dev, args):
    batch = tuple(t.to(dev) for t in mk(B, 500, c))
    engines = {"stage_one": getattr(E, cls)(c, B, device=dev, precision="bf16", lr=1e-3),
               "stage_two": getattr(E, cls)(c, B, device=dev, precision="bf16", lr=1e-3)}
    engines["stage_two"].freeze_modalities()
    replays = {k: e.capture(*batch) for k, e in engines.items()}
    times = {k: [] for k in replays}
    for fn in replays.values():
        events(lambda i: fn(), args.warmup)
    for _ in range(args.reps):
        for k, fn in replays.items():
            torch.cuda.synchronize()
            times[k].append(events(lambda i: fn(), args.steps))
    med, row = summary(times)
    return {"measure": "step", "case": name, "batch": B, "precision": "bf16", "steps": args.steps, "reps": args.reps, **row,
            "stage_two_over_stage_one": round(med["stage_two"] / med["stage_one"], 4),
            "trainable_params": sum(hi - lo for lo, hi in engines["stage_two"]._trainable), "params": engines["stage_two"].n_params}


def measure_gather(name, c, mk, B, dev, args):
    srcs = synthetic_split(mk, c, B, 16, dev)
    n = srcs[0].shape[0]
    order = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    plain = E.EpochFeed(srcs, B, dev)
    muted = E.EpochFeed(srcs, B, dev, muting=True)
    slots = plain.new_slots()
    ncodes = int(muted.mute_codes.numel())
    variants = {"plain": (plain, None), "code_0": (muted, 0), "mute_a": (muted, 1), "mute_b": (muted, 2)}
    times = {k: [] for k in variants}

    def start(feed, code):
        feed.start(order, muting=None if code is None else [code] * ncodes)

    def run(feed, code, steps):
        # (the schedule has 16 steps: restart it as often as the cursor wraps, so that every launch reads its code)
        total = 0.0
        for lo in range(0, steps, ncodes):
            start(feed, code)
            torch.cuda.synchronize()
            k = min(ncodes, steps - lo)
            total += events(lambda i: feed.gather_into(slots), k) * k
        return total / steps

    for feed, code in variants.values():
        run(feed, code, args.warmup)
    for _ in range(args.reps):
        for k, (feed, code) in variants.items():
            times[k].append(run(feed, code, args.steps))
    med, row = summary(times)
    row_bytes = [E.EpochFeed._row_bytes(s) * B for s in srcs]
    return {"measure": "gather", "case": name, "batch": B, "rows": n, "slot_bytes": sum(row_bytes), "source_bytes": row_bytes,
            "steps": args.steps, "reps": args.reps, **row, "code_0_over_plain": round(med["code_0"] / med["plain"], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("step", "gather"), default=None)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    def emit(row):
        row.update(device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    for name, cls, c, mk, B in CASES:
        if args.only in (None, "step"):
            emit(measure_step(name, cls, c, mk, B, dev, args))
    if args.only in (None, "gather"):
        name, cls, c, mk, B = CASES[0]
        emit(measure_gather(name, c, mk, B, dev, args))


if __name__ == "__main__":
    main()
