"""Step time of the evidential engine beside the cross-entropy engine: M2-Mixer-B, bf16, B = 512, the captured step of
AVMnistEngine and of AVMnistUQEngine alternated in one process and timed with device events.

    python scripts/edl_step_time.py [--rounds 7] [--steps 200] [--warmup 50]

Prints one JSON line: per engine the median over the rounds of the mean step time (ms), the minimum and maximum over the rounds,
and the difference of the medians in microseconds."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]

import torch  # noqa: E402

import gen_util as G  # noqa: E402
from m2_mixer_amd.engine import AVMnistEngine, AVMnistUQEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--batch", type=int, default=512)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(G.AVMNIST["B"])
    batch = tuple(t.to(dev) for t in G.avmnist_batch(a.batch, 7, cfg))
    replays = {}
    for name, cls in (("ce", AVMnistEngine), ("uq", AVMnistUQEngine)):
        eng = cls(cfg, a.batch, device=dev, precision="bf16", lr=1e-3, seed=3)
        replays[name] = (eng, eng.capture(*batch))
    times = {name: [] for name in replays}
    for _ in range(a.rounds):
        for name, (eng, replay) in replays.items():
            for _ in range(a.warmup):
                replay()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                replay()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / a.steps)
    out = {"config": "avmnist M2-Mixer-B bf16", "batch": a.batch, "rounds": a.rounds, "steps": a.steps}
    for name, ts in times.items():
        out[name] = {"median_ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}
    out["uq_minus_ce_us"] = round(1e3 * (out["uq"]["median_ms"] - out["ce"]["median_ms"]), 2)
    out["finite"] = all(bool(torch.isfinite(eng.losses).all()) for eng, _ in replays.values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
