"""Step time of the evidential engine beside the cross-entropy engine: M2-Mixer-B, bf16, B = 512, the captured step of
AVMnistEngine ("ce") and of AVMnistUQEngine alternated in one process and timed with device events.
The evidential engine is timed in its default form ("uq": squared-error risk, no KL term), with the cross-entropy Bayes risk ("uq_ce") and with that risk + the KL term at lambda = 1 ("uq_ce_kl": set_epoch(annealing_step)).

    python scripts/edl_step_time.py [--rounds 7] [--steps 200] [--warmup 50] [--edl-loss ce] [--kl-weight 1.0]

--edl-loss / --kl-weight: time that one form beside "ce" and "uq" instead of the two above.
Prints one JSON line: per engine the median over the rounds of the mean step time (ms), the minimum and maximum over the rounds,
and each evidential form's difference to "ce" (and to "uq") of the medians in microseconds."""
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
    ap.add_argument("--edl-loss", choices=("mse", "ce"), default=None)
    ap.add_argument("--kl-weight", type=float, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(G.AVMNIST["B"])
    batch = tuple(t.to(dev) for t in G.avmnist_batch(a.batch, 7, cfg))
    replays = {}
    forms = [("ce", AVMnistEngine, {}), ("uq", AVMnistUQEngine, {})]
    if a.edl_loss is not None or a.kl_weight is not None:
        loss, w = a.edl_loss or "mse", a.kl_weight or 0.0
        forms.append((f"uq_{loss}" + ("_kl" if w > 0 else ""), AVMnistUQEngine, dict(edl_loss=loss, kl_weight=w)))
    else:
        forms += [("uq_ce", AVMnistUQEngine, dict(edl_loss="ce")), ("uq_ce_kl", AVMnistUQEngine, dict(edl_loss="ce", kl_weight=1.0))]
    for name, cls, keys in forms:
        eng = cls(dict(cfg, **keys), a.batch, device=dev, precision="bf16", lr=1e-3, seed=3)
        if keys.get("kl_weight", 0.0) > 0:
            eng.set_epoch(eng.annealing_step)                  # lambda = kl_weight: the KL arithmetic runs
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
    for name in times:
        if name != "ce":
            out[f"{name}_minus_ce_us"] = round(1e3 * (out[name]["median_ms"] - out["ce"]["median_ms"]), 2)
        if name not in ("ce", "uq"):
            out[f"{name}_minus_uq_us"] = round(1e3 * (out[name]["median_ms"] - out["uq"]["median_ms"]), 2)
    out["finite"] = all(bool(torch.isfinite(eng.losses).all()) for eng, _ in replays.values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
