#!/usr/bin/env python3
"""Cost of the training accuracies: the training step with train_metrics off, on, and today's workaround (keep_logits +
step_outputs + content_accuracy + structure_metrics after every step), interleaved on one device (the arms rotate which goes
first), timed with device events over K steps per sample.  The metrics arm reads its history once per sample (a
`print_every` read), outside the timed window.

    python tools/train_metrics_ab.py [--d 256] [--batch 256] [--layers 8] [--rounds 12] [--steps 10] [--out FILE.json]
    python tools/train_metrics_ab.py --trace-only [--arm on] [--steps 8]   # 3 warm-up + K steps of one arm (the window of a
                                                                          # rocprofv3 kernel trace)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.model import VAE  # noqa: E402
from polyphemus_amd.synthetic import synthetic_batch  # noqa: E402
from polyphemus_amd.trainer import HipTrainer  # noqa: E402

ARMS = ("off", "on", "workaround")


def make(vae, arm, capacity):
    tr = HipTrainer(vae, lr=5e-6, train_metrics=arm == "on", metrics_capacity=capacity)
    tr.keep_logits = arm == "workaround"
    return tr


def step(tr, arm, batch, drum, s_t, sink):
    tr.train_step(batch)
    if arm == "workaround":                         # the route available without the option
        (s_logits, c_logits), _, _ = tr.step_outputs()
        full = torch.zeros(c_logits.shape[0], 15, 230, device=c_logits.device)
        full[:, :c_logits.shape[1]] = c_logits
        sink.append(torch.cat([ops.content_accuracy(full, batch.tokens, drum), ops.structure_metrics(s_t, s_t)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--arm", choices=ARMS, default="on", help="--trace-only: the arm traced")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=a.layers, d=a.d, n_bars=2, resolution=8, device=dev).to(dev)
    vae.train()
    batch = synthetic_batch(a.batch, 2, p=0.25, seed=a.seed).to(dev)
    batch.tokens = batch.tokens.to(torch.int32).contiguous()
    drum = (batch.is_drum.view(torch.uint8) if batch.is_drum.dtype == torch.bool else batch.is_drum).contiguous()
    s_t = batch.s_tensor.float().contiguous().reshape(-1)
    sink = []
    if a.trace_only:
        tr = make(vae, a.arm, a.steps + 3)
        for _ in range(3):
            step(tr, a.arm, batch, drum, s_t, sink)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            step(tr, a.arm, batch, drum, s_t, sink)
        torch.cuda.synchronize()
        acc = tr.read_train_accuracies()[-1] if a.arm == "on" else None
        print(json.dumps({"trace_only": True, "arm": a.arm, "steps": a.steps, "last_accuracies": acc}))
        return
    trainers = {k: make(vae, k, max(a.steps, 3)) for k in ARMS}
    for k, tr in trainers.items():                   # warm-up: code objects, arenas, plan buffers
        for _ in range(3):
            step(tr, k, batch, drum, s_t, sink)
        if k == "on":
            tr.read_train_accuracies()
    torch.cuda.synchronize()
    samples = {k: [] for k in ARMS}
    for r in range(a.rounds):
        order = ARMS[r % 3:] + ARMS[:r % 3]
        for k in order:
            tr = trainers[k]
            sink.clear()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                step(tr, k, batch, drum, s_t, sink)
            e1.record()
            e1.synchronize()
            samples[k].append(1e3 * e0.elapsed_time(e1) / a.steps)          # us per step
            if k == "on":
                last = tr.read_train_accuracies()[-1]
    med = {k: statistics.median(v) for k, v in samples.items()}
    diff = {k: [x - o for o, x in zip(samples["off"], samples[k])] for k in ("on", "workaround")}
    res = {"config": {"d": a.d, "batch": a.batch, "layers": a.layers, "n_bars": 2, "batch_seed": a.seed,
                      "nodes": batch.num_nodes, "rounds": a.rounds, "steps_per_sample": a.steps},
           "us_per_step_median": {k: round(v, 1) for k, v in med.items()},
           **{f"{k}_minus_off_us": {"median_of_round_pairs": round(statistics.median(v), 1), "min": round(min(v), 1),
                                    "max": round(max(v), 1)} for k, v in diff.items()},
           "relative_on": round(statistics.median(diff["on"]) / med["off"], 5),
           "samples_us": {k: [round(x, 1) for x in v] for k, v in samples.items()},
           "last_accuracies": last}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
