#!/usr/bin/env python3
"""What a captured evaluation pass saves over the eager fed pass, with and without a prediction record: one JSON line per arm
(DESIGN.md section 16).

M2-Mixer-B, bf16, batch 512, a synthetic resident split of 5000 rows (AV-MNIST's validation split: nine full batches and a tail
of 392).  Three arms, each with and without a record, on ONE engine:
  eager       data.run_epoch_fed(train=False, replay=None): every step launched from Python (the path before captured evaluation)
  captured_1  ... replay=engine.capture_feed_eval(feed, steps=1): nine replays and the tail
  captured_3  ... steps=3: three replays and the tail
A pass is one run_epoch_fed call and ends in its one synchronisation (feed.read()).  Per repetition and arm: --warmup untimed
passes, then --passes timed ones (wall clock around all of them); the arms are ALTERNATED within a repetition, --reps
repetitions, and an arm's figure is its best repetition (all repetitions are kept in the row).

A row of `calls` per engine class counts the launching library calls of one eager evaluation step, with and without a record
(what a captured step consists of; m2m_feed_gather and m2m_record_append are two launches each, a tower forward on the wide path
is several, every other call here is one; host-side predicates are not counted).

--arm NAME runs that arm alone, untimed (--warmup + --passes passes): the form to put under `rocprofv3 --kernel-trace`.
--trace-csv FILE --arm NAME then prints one `trace` row from that run's kernel trace: per pass (the last --passes ones; a pass is
ten gather launches) the kernels, the time from the first kernel's start to the last one's end, the sum of the kernel times and
what is left between them -- medians over the passes.

Usage: python scripts/eval_feed_overhead.py [--passes 20] [--warmup 3] [--reps 3] [--out profiles/eval_feed.jsonl]"""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from scores_overhead import CASES, E                      # noqa: E402
from feed_overhead import synthetic_split                 # noqa: E402
from m2_mixer_amd import _lib as L                        # noqa: E402
from m2_mixer_amd import data as D                        # noqa: E402

ROWS, BATCH, CAPACITY = 5000, 512, 8192
# calls that launch nothing: host-side predicates, and the recording half of the riding MLP (the time tower's token-mixing launch
# carries it, or m2m_mlp_ride_flush launches it)
PREDICATES = ("m2m_mlp_forward_ride", "m2m_towers_can_group", "m2m_towers_forward_embeds_ok", "m2m_tower_backward_heads_ok", "m2m_embed_fwd_splits",
              "m2m_heads_part_tiles", "m2m_wgrad_form", "m2m_split_form", "m2m_pack_skips_w1tc", "m2m_abi_version")


class _CountingLib:
    """The loaded library with every m2m_* call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("m2m_") or name == "m2m_last_error":
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)

        return counted


def count_calls(name, cls, c, mk, B, dev):
    """Library calls of one fed evaluation step (gather, evaluate, accumulate), without and with a record."""
    eng = getattr(E, cls)(c, B, device=dev, precision="bf16", lr=1e-3)
    feed = E.EpochFeed(tuple(t.to(dev).contiguous() for t in mk(2 * B, 7, c)), B, dev, uncertainty=hasattr(eng, "uncertainty"))
    feed.bind(eng)
    feed.start()
    slots, rec, out = feed.new_slots(), eng.new_prediction_record(2 * B), {}
    real = L.lib()
    for tag, record in (("plain", None), ("record", rec)):
        L._lib = proxy = _CountingLib(real)
        try:
            feed.gather_into(slots)
            eng.evaluate(*slots, record=record)
            feed.accumulate(eng, slots[-1])
        finally:
            L._lib = real
        out[tag] = {k: v for k, v in sorted(proxy.calls.items()) if k not in PREDICATES}
        out[tag + "_launching_calls"] = sum(out[tag].values())
    torch.cuda.synchronize()
    return {"measure": "calls", "case": name, "engine": cls, "batch": B, **out}


def trace_row(path, arm, passes):
    """One `trace` row from a rocprofv3 --kernel-trace csv of an --arm run."""
    import csv
    import statistics
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    heads = [i for i, r in enumerate(rows) if "feed_gather_kernel" in r["Kernel_Name"]]
    per_pass = (ROWS + BATCH - 1) // BATCH
    heads = heads[-passes * per_pass:][::per_pass]                        # the first gather of each of the last passes
    assert len(heads) == passes, (len(heads), passes)
    spans, busy, kernels = [], [], []
    for a, b in zip(heads, heads[1:] + [len(rows)]):
        seg = rows[a:b]
        while "feed_gather_kernel" not in seg[-1]["Kernel_Name"] and any(
                k in seg[-1]["Kernel_Name"] for k in ("fill", "Fill", "copy", "Copy")):
            seg = seg[:-1]                                                  # (the next pass's resets: fills and copies of feed.start)
        spans.append((max(int(r["End_Timestamp"]) for r in seg) - int(seg[0]["Start_Timestamp"])) / 1e3)
        busy.append(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seg) / 1e3)
        kernels.append(len(seg))
    med = statistics.median
    return {"measure": "trace", "arm": arm, "passes": passes, "kernels_per_pass": med(kernels), "span_us": round(med(spans), 1),
            "kernel_sum_us": round(med(busy), 1), "between_kernels_us": round(med(spans) - med(busy), 1)}


def measure(dev, args):
    name, cls, c, mk, _ = CASES[0]
    assert name == "avmnist_B"
    full = synthetic_split(mk, c, BATCH, (ROWS + BATCH - 1) // BATCH, dev)
    srcs = tuple(t[:ROWS].contiguous() for t in full)
    eng = getattr(E, cls)(c, BATCH, device=dev, precision="bf16", lr=1e-3)
    feed = E.EpochFeed(srcs, BATCH, dev)
    tail = eng.sibling(ROWS % BATCH, trains=False)
    rec = eng.prediction_record("val", CAPACITY)
    plan = {k: D.feed_plan(ROWS, BATCH, k) for k in (1, 3)}
    arms = {}
    for record in (None, rec):
        tag = "" if record is None else "+record"
        arms["eager" + tag] = (None, record)
        for k in (1, 3):
            arms[f"captured_{k}{tag}"] = (eng.capture_feed_eval(feed, steps=k, record=record), record)

    def one_pass(arm):
        replay, record = arms[arm]
        return D.run_epoch_fed(eng, feed, replay, train=False, split="val", record=record, tail_engine=tail)

    if args.arm:                                           # one arm alone, untimed: the run to trace
        for _ in range(args.warmup + args.passes):
            one_pass(args.arm)
        torch.cuda.synchronize()
        return []
    ref = one_pass("eager")
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for arm in arms:                                   # alternated: every arm once per repetition
            for _ in range(args.warmup):
                out = one_pass(arm)
            assert out["samples"] == ROWS and out["steps"] == 10 and abs(out["loss"] - ref["loss"]) < 1e-5 * abs(ref["loss"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.passes):
                one_pass(arm)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) / args.passes)
    assert rec.rows() == ROWS
    rows = []
    for arm, v in times.items():
        base = times["eager+record" if arm.endswith("+record") else "eager"]
        steps = int(arm.split("_")[1].split("+")[0]) if arm.startswith("captured") else 0
        rows.append({"measure": "eval_pass", "case": name, "arm": arm, "record": arm.endswith("+record"), "precision": "bf16",
                     "batch": BATCH, "rows": ROWS, "plan": list(plan[steps]) if steps else [0, ROWS // BATCH, ROWS % BATCH],
                     "passes": args.passes, "warmup": args.warmup, "reps": args.reps,
                     "best_ms_per_pass": round(min(v) * 1e3, 4), "reps_ms_per_pass": [round(x * 1e3, 4) for x in v],
                     "spread_ms": round((max(v) - min(v)) * 1e3, 4), "samples_per_s": round(ROWS / min(v), 1),
                     "over_eager": round(min(v) / min(base), 4)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eval_feed.jsonl"))
    ap.add_argument("--only", choices=("calls", "eval_pass"), default=None)
    ap.add_argument("--arm", default=None, help="run this arm alone, untimed (eager, captured_1, captured_3, each also +record)")
    ap.add_argument("--trace-csv", default=None, help="a rocprofv3 --kernel-trace csv of an --arm run: print its `trace` row")
    args = ap.parse_args()
    if args.trace_csv:
        print(json.dumps(trace_row(args.trace_csv, args.arm, args.passes)))
        return
    if not torch.cuda.is_available():
        raise SystemExit("eval_feed_overhead: needs the GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    rows = []
    if args.arm:
        measure(dev, args)
        return
    if args.only in (None, "eval_pass"):
        rows += measure(dev, args)
    if args.only in (None, "calls"):
        rows += [count_calls(*case, dev) for case in CASES]
        name, _, c, mk, B = CASES[0]
        rows.append(count_calls(name + "_uq", "AVMnistUQEngine", c, mk, B, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            row.update(device=torch.cuda.get_device_name(0), csrc=L.csrc_hash()[:16])
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
