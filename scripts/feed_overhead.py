#!/usr/bin/env python3
"""What the epoch feed costs and returns: one JSON line per measurement.

  gather  m2m_feed_gather alone, filling one step's input slots from a shuffled resident split of 16 batches, against the two
          other ways to fill the same slots: `select_copy` = one index_select + one copy_ per source (how a shuffled batch
          reaches the slots of engine.capture's replay) and `copy` = a plain copy_ of the same bytes from a contiguous block
          (the bound of any copy; reported as achieved bytes/s, read + written).  HIP events around --steps launches after
          --warmup, --reps repetitions with the variants INTERLEAVED repetition by repetition in one process; medians and
          the spread (max - min over the repetitions) of each.
  epoch   a whole training epoch of --batches batches on a synthetic resident split, bf16: `loop` = the host loop (AV-MNIST:
          data.run_epoch with its replay, unshuffled, the only training order it has; the others: capture() + replay(index_select
          ...) over a shuffled order with run_epoch's three accumulating torch ops) against data.run_epoch_fed over a shuffled
          order with a 1-step and a 4-step fed graph -- all on ONE engine.  Wall clock around the epoch (its read-back
          included), --reps repetitions interleaved, medians, samples/s.

Shapes: M2-Mixer-B at batch 512, MIMIC-H at 128, MM-IMDb at 32.
Usage: python scripts/feed_overhead.py [--steps 200] [--warmup 20] [--reps 5] [--batches 64] [--only gather|epoch] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scores_overhead import CASES, E                      # noqa: E402
from m2_mixer_amd import data as D                        # noqa: E402


def synthetic_split(mk, c, B, nbatches, dev):
    """nbatches x B samples: one seeded batch per B rows (the generators build a batch at a time)."""
    parts = [mk(B, 500 + i, c) for i in range(nbatches)]
    return tuple(torch.cat([p[k] for p in parts]).to(dev).contiguous() for k in range(len(parts[0])))


def events(fn, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(steps):
        fn(i)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / steps


def measure_gather(name, c, mk, B, dev, args):
    srcs = synthetic_split(mk, c, B, 16, dev)
    n = srcs[0].shape[0]
    feed = E.EpochFeed(srcs, B, dev)
    order = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    slots = feed.new_slots()
    nb = n // B

    def select_copy(i):
        idx = order[(i % nb) * B:(i % nb + 1) * B]
        for s, t in zip(srcs, slots):
            t.copy_(s.index_select(0, idx), non_blocking=True)

    def copy(i):
        lo = (i % nb) * B
        for s, t in zip(srcs, slots):
            t.copy_(s[lo:lo + B], non_blocking=True)

    variants = {"feed": lambda i: feed.gather_into(slots), "select_copy": select_copy, "copy": copy}
    times = {k: [] for k in variants}
    for k, fn in variants.items():
        feed.start(order)
        events(fn, args.warmup)
    for _ in range(args.reps):
        for k, fn in variants.items():
            feed.start(order)                              # (the cursor wraps every 16 launches: the same rows, in-bounds)
            torch.cuda.synchronize()
            times[k].append(events(fn, args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = 2 * sum(E.EpochFeed._row_bytes(s) for s in srcs) * B
    return {"measure": "gather", "case": name, "batch": B, "rows": n, "slot_bytes": moved // 2, "steps": args.steps, "reps": args.reps,
            **{k + "_us": round(v * 1e3, 2) for k, v in med.items()},
            **{k + "_spread_us": round((max(v) - min(v)) * 1e3, 2) for k, v in times.items()},
            **{k + "_GBps": round(moved / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
            "feed_over_select_copy": round(med["feed"] / med["select_copy"], 4),
            **{k + "_reps_us": [round(x * 1e3, 2) for x in v] for k, v in times.items()}}


class _AVSplits(D.ResidentAVMnist):
    """ResidentAVMnist over tensors that are already resident (no files)."""

    def __init__(self, splits, device):
        self.device, self.rank, self.world, self.splits = torch.device(device), 0, 1, splits


def measure_epoch(name, cls, c, mk, B, dev, args):
    srcs = synthetic_split(mk, c, B, args.batches, dev)
    n = srcs[0].shape[0]
    eng = getattr(E, cls)(c, B, device=dev, precision="bf16", lr=1e-3)
    feed = E.EpochFeed(srcs, B, dev)
    plain = eng.capture(*(t[:B] for t in srcs))
    fed = {1: eng.capture_feed(feed, steps=1), 4: eng.capture_feed(feed, steps=4)}
    gen = torch.Generator(device=dev).manual_seed(2)
    av = _AVSplits({"train": srcs}, dev) if name == "avmnist_B" else None

    def loop():
        if av is not None:
            return D.run_epoch(eng, av, "train", B, train=True, replay=plain, log_interval_steps=10 ** 9)
        order = torch.randperm(n, device=dev, generator=gen)
        acc = torch.zeros(11, device=dev, dtype=torch.float64)
        for lo in range(0, n, B):
            idx = order[lo:lo + B]
            batch = tuple(t.index_select(0, idx) for t in srcs)
            plain(*batch)
            acc[:4] += eng.losses
            acc[4:8] += eng.losses * B
            if eng.preds.dim() == 2:
                acc[8:11] += (eng.preds == batch[-1].to(eng.preds.dtype)[None, :]).sum(dim=1)
        return acc.cpu()

    def fed_epoch(k):
        return D.run_epoch_fed(eng, feed, fed[k], n, order=torch.randperm(n, device=dev, generator=gen))

    variants = {"loop": loop, "fed_1": lambda: fed_epoch(1), "fed_4": lambda: fed_epoch(4)}
    times = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    for _ in range(args.reps):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"measure": "epoch", "case": name, "batch": B, "batches": args.batches, "samples": n, "precision": "bf16", "reps": args.reps,
            "loop_order": "unshuffled (run_epoch)" if av is not None else "shuffled",
            **{k + "_samples_per_s": round(n / v, 1) for k, v in med.items()},
            **{k + "_ms_per_batch": round(v / args.batches * 1e3, 4) for k, v in med.items()},
            **{k + "_reps_ms": [round(x * 1e3, 3) for x in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--only", choices=("gather", "epoch"), default=None)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        row.update(device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        rows.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    for name, cls, c, mk, B in CASES:
        if args.only in (None, "gather"):
            emit(measure_gather(name, c, mk, B, dev, args))
    for name, cls, c, mk, B in CASES:
        if args.only in (None, "epoch"):
            emit(measure_epoch(name, cls, c, mk, B, dev, args))


if __name__ == "__main__":
    main()
