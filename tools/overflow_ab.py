#!/usr/bin/env python3
"""Cost of the guarded optimizer step: the training step with overflow="ignore" against overflow="skip" on the same model and
batch, interleaved on one device (rounds alternate which policy goes first), timed with device events over K steps per sample.

    python tools/overflow_ab.py [--d 256] [--batch 256] [--layers 8] [--rounds 12] [--steps 10] [--out FILE.json]
    python tools/overflow_ab.py --trace-only [--policy skip] [--steps 8]   # 3 warm-up + K steps of one policy (the window
                                                                          # of a rocprofv3 kernel / HIP API trace)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polyphemus_amd.model import VAE  # noqa: E402
from polyphemus_amd.synthetic import synthetic_batch  # noqa: E402
from polyphemus_amd.trainer import HipTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--policy", choices=("ignore", "skip"), default="skip", help="--trace-only: the policy traced")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=a.layers, d=a.d, n_bars=2, resolution=8, device=dev).to(dev)
    vae.train()
    batch = synthetic_batch(a.batch, 2, p=0.25, seed=a.seed).to(dev)
    if a.trace_only:
        tr = HipTrainer(vae, lr=5e-6, overflow=a.policy)
        for _ in range(3):
            tr.train_step(batch)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            tr.train_step(batch)
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "policy": a.policy, "steps": a.steps, "overflow_stats": tr.overflow_stats()}))
        return
    skip = HipTrainer(vae, lr=5e-6, overflow="skip")
    ignore = HipTrainer(vae, lr=5e-6)
    trainers = {"ignore": ignore, "skip": skip}
    for tr in trainers.values():                     # warm-up: code objects, arenas, plan buffers
        for _ in range(3):
            tr.train_step(batch)
    torch.cuda.synchronize()
    samples = {k: [] for k in trainers}
    for r in range(a.rounds):
        order = ("ignore", "skip") if r % 2 == 0 else ("skip", "ignore")
        for k in order:
            tr = trainers[k]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                tr.train_step(batch)
            e1.record()
            e1.synchronize()
            samples[k].append(1e3 * e0.elapsed_time(e1) / a.steps)          # us per step
    med = {k: statistics.median(v) for k, v in samples.items()}
    pair = [s - i for i, s in zip(samples["ignore"], samples["skip"])]
    res = {"config": {"d": a.d, "batch": a.batch, "layers": a.layers, "n_bars": 2, "batch_seed": a.seed,
                      "nodes": batch.num_nodes, "rounds": a.rounds, "steps_per_sample": a.steps},
           "us_per_step_median": {k: round(v, 1) for k, v in med.items()},
           "skip_minus_ignore_us": {"median_of_round_pairs": round(statistics.median(pair), 1),
                                    "min": round(min(pair), 1), "max": round(max(pair), 1)},
           "relative": round(statistics.median(pair) / med["ignore"], 5),
           "samples_us": {k: [round(x, 1) for x in v] for k, v in samples.items()},
           "skipped_steps": int(skip.skipped_steps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
