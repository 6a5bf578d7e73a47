#!/usr/bin/env python3
"""What the ranking buffers cost: one JSON line per measurement.

  step    the captured training step with rank_scores=True and False (and, with --parent-root, the parent commit's engine), bf16,
          HIP events around --steps replays after --warmup, --reps repetitions with the variants INTERLEAVED repetition by
          repetition in one process; medians.  Cases: MIMIC-H at its cfg batch 128, M2-Mixer-B at batch 512.  The buffer is
          emptied before every timed run (an overflowing append writes nothing and would be cheaper).
  counts  m2m_rank_counts alone on a buffer of n random softmax rows, K classes, 3 heads: HIP events around one launch, --reps
          launches after one, median.  Sizes: the AV-MNIST training split (55 000 rows, K = 10) and MIMIC's (28 970 = the
          36 212 samples of MultiBench's im.pk less the fifth datasets/mimic.py:82-89 holds out, K = 6).

--parent-root DIR: a checkout of the parent commit with its library built (scripts/scores_overhead.py loads it the same way); adds
the parent's engine and a second rank_scores=False engine built after it to the interleaved variants.
Usage: python scripts/rank_overhead.py [--steps 200] [--warmup 20] [--reps 5] [--parent-root DIR] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scores_overhead import G, E, load_parent, prepare, timed          # noqa: E402

STEP_CASES = [("mimic_H", "MimicEngine", G.MIMIC_H, G.mimic_batch, 128), ("avmnist_B", "AVMnistEngine", G.AVMNIST["B"], G.avmnist_batch, 512)]
COUNT_CASES = [("avmnist_train", 55000, 10), ("mimic_train", 28970, 6)]


def time_counts(n, K, reps, dev):
    rb = E.RankBuffer("mimic", ("a", "b", "fusion"), K, 65536, dev)
    gen = torch.Generator(device=dev).manual_seed(n + K)
    rb.probs[:, :, :n] = torch.softmax(torch.randn(3, n, K, generator=gen, device=dev) * 2, dim=2).transpose(1, 2)
    rb.labels[:n] = torch.randint(0, K, (n,), generator=gen, device=dev, dtype=torch.int32)
    out = torch.zeros(3, n, 4, dtype=torch.int32, device=dev)
    from m2_mixer_amd import _lib as L
    ms = []
    for i in range(reps + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        L.check(L.lib().m2m_rank_counts(rb.probs.data_ptr(), rb.labels.data_ptr(), 3, n, K, rb.capacity, out.data_ptr(), L.stream_ptr()), "rank_counts")
        e.record()
        e.synchronize()
        if i:
            ms.append(s.elapsed_time(e))
    assert int(out[:, :, 0].min()) >= 1 and int(out[:, :, 0].max()) <= n
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        row.update(device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        rows.append(row)

    parent = load_parent(args.parent_root) if args.parent_root else None
    for name, cls, c, mk, B in STEP_CASES:
        variants = {"rank_on": prepare(E, cls, c, mk, B, dev, args, rank_scores=True, rank_capacity=max(65536, args.steps * B)),
                    "rank_off": prepare(E, cls, c, mk, B, dev, args)}
        if parent is not None:
            variants["parent"] = prepare(parent, cls, c, mk, B, dev, args)
            # two engines of the same code differ by where their buffers landed: a second rank_scores=False
            # engine, built AFTER the parent's, shows the spread the parent's figure has to sit within
            variants["rank_off_built_after_parent"] = prepare(E, cls, c, mk, B, dev, args)
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, (eng, replay, batches) in variants.items():
                if getattr(eng, "rank", None) is not None:
                    eng.rank.reset()                       # (the capacity holds steps x B rows: every append writes)
                times[k].append(timed(replay, batches, args.steps))
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"measure": "step", "case": name, "batch": B, "precision": "bf16", "steps": args.steps, "reps": args.reps,
               **{k + "_ms": round(v, 4) for k, v in med.items()}, "added_us": round((med["rank_on"] - med["rank_off"]) * 1e3, 2),
               **{k + "_reps_ms": [round(x, 4) for x in v] for k, v in times.items()}}
        emit(row)
        del variants
    for name, n, K in COUNT_CASES:
        ms = time_counts(n, K, args.reps, dev)
        emit({"measure": "counts", "case": name, "n": n, "K": K, "nheads": 3, "compares": 3 * n * n, "median_ms": round(statistics.median(ms), 4),
              "reps_ms": [round(x, 4) for x in ms]})
    if args.out:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
