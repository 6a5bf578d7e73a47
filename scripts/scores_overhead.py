#!/usr/bin/env python3
"""What the scores launch costs in the captured training step: one JSON line per case with the replayed step's ms with
scores=True and with scores=False (HIP events around --steps replays after --warmup, best of --reps, the two variants alternated
repetition by repetition in ONE process) and their ratio.  bf16, dropout as in the cfg.  Cases: M2-Mixer-B at batch 512,
MIMIC-H at 128, MM-IMDb at 32.
--parent-root DIR: a checkout of the parent commit with its library built (make -C DIR/m2_mixer_amd/csrc); adds a row that times
this tree's scores=False engine against the parent's engine at M2-Mixer-B the same way (loaded as a second package in the same
process) -- nothing was added to that step, so the ratio must sit within run-to-run spread.
Usage: python scripts/scores_overhead.py [--steps 200] [--warmup 20] [--reps 3] [--only CASE] [--parent-root DIR] [--out FILE]
(--only avmnist_B --variant on: that one engine alone, e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import gen_util as G                           # noqa: E402
from m2_mixer_amd import engine as E           # noqa: E402

CASES = [("avmnist_B", "AVMnistEngine", G.AVMNIST["B"], G.avmnist_batch, 512), ("mimic_H", "MimicEngine", G.MIMIC_H, G.mimic_batch, 128),
         ("mmimdb", "MMIMDBEngine", G.MMIMDB, G.mmimdb_batch, 32)]


def load_parent(root):
    """The parent checkout's package under another name (its own libm2mixer.so next to it)."""
    path = os.path.join(root, "m2_mixer_amd")
    spec = importlib.util.spec_from_file_location("m2_mixer_parent", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["m2_mixer_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("m2_mixer_parent.engine")


def prepare(engine_mod, cls, c, mk, B, dev, args, **kw):
    eng = getattr(engine_mod, cls)(c, B, device=dev, precision="bf16", lr=1e-3, **kw)
    batches = [[t.to(dev) for t in mk(B, 100 + i, c)] for i in range(4)]
    replay = eng.capture(*batches[0])
    for i in range(args.warmup):
        replay(*batches[i % 4])
    torch.cuda.synchronize()
    return eng, replay, batches


def timed(replay, batches, steps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(steps):
        replay(*batches[i % 4])
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / steps


def alternate(variants, args):
    """reps x (each variant in turn): per-variant lists of ms per step."""
    times = [[] for _ in variants]
    for _ in range(args.reps):
        for t, v in zip(times, variants):
            t.append(timed(v[1], v[2], args.steps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--variant", choices=("on", "off"), default=None, help="with --only: run that engine alone (profiling)")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        row.update(precision="bf16", steps=args.steps, reps=args.reps, device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        rows.append(row)

    for name, cls, c, mk, B in CASES:
        if args.only and args.only != name:
            continue
        if args.variant:
            _, replay, batches = prepare(E, cls, c, mk, B, dev, args, scores=args.variant == "on")
            emit({"case": name, "batch": B, "variant": "scores_" + args.variant, "step_ms": round(timed(replay, batches, args.steps), 4)})
            continue
        on = prepare(E, cls, c, mk, B, dev, args, scores=True)
        off = prepare(E, cls, c, mk, B, dev, args, scores=False)
        t_on, t_off = alternate((on, off), args)
        emit({"case": name, "batch": B, "compare": "scores_on / scores_off", "on_ms": round(min(t_on), 4), "off_ms": round(min(t_off), 4),
              "ratio": round(min(t_on) / min(t_off), 4), "added_us": round((min(t_on) - min(t_off)) * 1e3, 2),
              "on_reps_ms": [round(x, 4) for x in t_on], "off_reps_ms": [round(x, 4) for x in t_off]})
        if name == "avmnist_B" and args.parent_root:
            # a second scores=False engine built AFTER the parent's: two engines of the same code differ by where their buffers
            # landed, which is the spread the parent's figure has to sit within
            parent = prepare(load_parent(args.parent_root), cls, c, mk, B, dev, args)
            off2 = prepare(E, cls, c, mk, B, dev, args, scores=False)
            t_off1, t_par, t_off2 = alternate((off, parent, off2), args)
            emit({"case": name, "batch": B, "compare": "scores_off / parent commit", "off_ms": round(min(t_off1), 4),
                  "parent_ms": round(min(t_par), 4), "off_built_after_parent_ms": round(min(t_off2), 4),
                  "ratio": round(min(t_off1) / min(t_par), 4), "ratio_built_after": round(min(t_off2) / min(t_par), 4),
                  "off_reps_ms": [round(x, 4) for x in t_off1], "parent_reps_ms": [round(x, 4) for x in t_par],
                  "off_built_after_reps_ms": [round(x, 4) for x in t_off2]})
            del parent, off2
        del on, off
    if args.out:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
