#!/usr/bin/env python3
"""Cost of clipping the gradient by its global norm: the training step of trainers that differ only in `max_grad_norm` /
`overflow`, on the same model and batch, interleaved on one device (rounds alternate the order), timed with device events over
K steps per sample.  Variants: none (max_grad_norm=None, "ignore"), inf_ignore, clip_ignore (1.0), clip_skip (1.0, "skip") and
skip (None, "skip": what clip_skip is compared with; the fifth trainer beside the four variants of the option).  All trainers
update the same model, as in tools/overflow_ab.py: the clipping ones take smaller steps on the shared parameters than the others,
which changes no launch and no byte count, so the timing is unaffected.

    python tools/clip_ab.py [--d 256] [--batch 256] [--layers 8] [--rounds 12] [--steps 10] [--out FILE.json]
    python tools/clip_ab.py --trace-only [--variant clip_skip] [--steps 8]   # 3 warm-up + K steps of one variant (the window
                                                                            # of a rocprofv3 kernel trace)
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

VARIANTS = {"none": dict(), "inf_ignore": dict(max_grad_norm=float("inf")), "clip_ignore": dict(max_grad_norm=1.0),
            "clip_skip": dict(max_grad_norm=1.0, overflow="skip"), "skip": dict(overflow="skip")}
PAIRS = [("inf_ignore", "none"), ("clip_ignore", "none"), ("clip_skip", "none"), ("skip", "none"), ("clip_skip", "skip")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--variant", choices=tuple(VARIANTS), default="clip_skip", help="--trace-only: the variant traced")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=a.layers, d=a.d, n_bars=2, resolution=8, device=dev).to(dev)
    vae.train()
    batch = synthetic_batch(a.batch, 2, p=0.25, seed=a.seed).to(dev)
    if a.trace_only:
        tr = HipTrainer(vae, lr=5e-6, **VARIANTS[a.variant])
        for _ in range(3):
            tr.train_step(batch)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            tr.train_step(batch)
        torch.cuda.synchronize()
        rows = tr.read_grad_norms() if tr.max_grad_norm is not None else []
        print(json.dumps({"trace_only": True, "variant": a.variant, "steps": a.steps, "grad_norms": rows[-2:],
                          "overflow_stats": tr.overflow_stats()}))
        return
    cap = 3 + a.rounds * a.steps
    trainers = {k: HipTrainer(vae, lr=5e-6, grad_norm_capacity=cap, **kw) for k, kw in VARIANTS.items()}
    for tr in trainers.values():                     # warm-up: code objects, arenas, plan buffers
        for _ in range(3):
            tr.train_step(batch)
    torch.cuda.synchronize()
    samples = {k: [] for k in trainers}
    names = list(trainers)
    for r in range(a.rounds):
        order = names[r % len(names):] + names[:r % len(names)]     # every variant takes every position
        if r % 2:
            order.reverse()
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
    diffs = {}
    for x, y in PAIRS:
        pair = [p - q for p, q in zip(samples[x], samples[y])]
        diffs[f"{x}_minus_{y}_us"] = {"median_of_round_pairs": round(statistics.median(pair), 1),
                                      "min": round(min(pair), 1), "max": round(max(pair), 1)}
    norms = trainers["clip_skip"].read_grad_norms()
    res = {"config": {"d": a.d, "batch": a.batch, "layers": a.layers, "n_bars": 2, "batch_seed": a.seed,
                      "nodes": batch.num_nodes, "params": vae.flat_params.numel(), "rounds": a.rounds,
                      "steps_per_sample": a.steps},
           "us_per_step_median": {k: round(v, 1) for k, v in med.items()},
           "differences": diffs,
           "samples_us": {k: [round(x, 1) for x in v] for k, v in samples.items()},
           "last_norm_coef": norms[-1] if norms else None,
           "skipped_steps": {k: int(trainers[k].skipped_steps) for k in ("clip_skip", "skip")}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
