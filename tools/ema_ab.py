#!/usr/bin/env python3
"""Cost of the parameter average: the training step at BASELINE configs[1] (d = 256, B = 256, 8 layers, 2 bars) three ways on
the same model and batch —
    off    HipTrainer(ema_decay=None)
    ema    HipTrainer(ema_decay=0.999): the average rides in the Adam launch
    lerp   HipTrainer(ema_decay=None) and `torch.lerp_` of a second buffer towards vae.flat_params behind every step: the
           alternative the kernel replaces
and `off2`, a second trainer like `off`: the difference off2 - off is the box's run-to-run spread, the yardstick for the other
differences.  Interleaved on one device in one process (every round runs all four, the order rotates), timed with device events
over K steps per sample after a warm-up; medians over rounds * K steps per variant.  Also the Adam launch alone at the model's
parameter count (back-to-back launches between two events: launch-bound work would show the launch rate, this pass is not).

    python tools/ema_ab.py [--d 256] [--batch 256] [--layers 8] [--rounds 40] [--steps 10] [--out FILE.json]
    python tools/ema_ab.py --trace-only [--variant ema] [--steps 8]     # 3 warm-up + K steps of one variant (the window of a
                                                                        # rocprofv3 --kernel-trace --stats run)
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

DECAY = 0.999
VARIANTS = ("off", "ema", "lerp", "off2")


class Variant:
    def __init__(self, name, vae):
        self.name = name
        self.tr = HipTrainer(vae, lr=5e-6, ema_decay=DECAY if name == "ema" else None)
        self.avg = vae.flat_params.detach().clone() if name == "lerp" else None
        self.flat = vae.flat_params.detach()

    def step(self, batch):
        self.tr.train_step(batch)
        if self.avg is not None:
            self.avg.lerp_(self.flat, 1.0 - DECAY)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps                            # us per call


def adam_launch_times(n, dev, samples=15, reps=200):
    """us per launch of the Adam pass over n parameters: plain, with the average, and the stand-alone lerp_ pass"""
    g = torch.Generator(device=dev).manual_seed(1)
    p, grad, e = (torch.randn(n, device=dev, generator=g) for _ in range(3))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    w = ops.ema_weight(DECAY)
    fns = {"adam": lambda: ops.adam_step(p, grad, m, v, 5e-6, 0.9, 0.98, 1e-9, 1),
           "adam_ema": lambda: ops.adam_step_ema(p, grad, m, v, e, 5e-6, 0.9, 0.98, 1e-9, 1, w),
           "lerp_": lambda: e.lerp_(p, 1.0 - DECAY)}
    out = {k: [] for k in fns}
    for k, fn in fns.items():
        timed(fn, 20)
    for s in range(samples):
        for k in (list(fns) if s % 2 == 0 else list(fns)[::-1]):
            out[k].append(timed(fns[k], reps))
    return {k: round(statistics.median(x), 2) for k, x in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--variant", choices=VARIANTS[:3], default="ema", help="--trace-only: the variant traced")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=a.layers, d=a.d, n_bars=2, resolution=8, device=dev).to(dev)
    vae.train()
    batch = synthetic_batch(a.batch, 2, p=0.25, seed=a.seed).to(dev)
    if a.trace_only:
        var = Variant(a.variant, vae)
        for _ in range(3):
            var.step(batch)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            var.step(batch)
        torch.cuda.synchronize()
        print(json.dumps({"trace_only": True, "variant": a.variant, "steps": a.steps}))
        return
    variants = {k: Variant(k, vae) for k in VARIANTS}
    for var in variants.values():                    # warm-up: code objects, arenas, plan buffers
        for _ in range(5):
            var.step(batch)
    torch.cuda.synchronize()
    samples = {k: [] for k in VARIANTS}
    for r in range(a.rounds):
        order = VARIANTS[r % 4:] + VARIANTS[:r % 4]
        for k in order:
            samples[k].append(timed(lambda: variants[k].step(batch), a.steps))
    med = {k: statistics.median(v) for k, v in samples.items()}

    def pairs(x, y):
        d = [s - i for i, s in zip(samples[y], samples[x])]
        return {"median_of_round_pairs": round(statistics.median(d), 1), "min": round(min(d), 1), "max": round(max(d), 1)}

    res = {"config": {"d": a.d, "batch": a.batch, "layers": a.layers, "n_bars": 2, "batch_seed": a.seed,
                      "nodes": batch.num_nodes, "params": vae.flat_params.numel(), "decay": DECAY, "rounds": a.rounds,
                      "steps_per_sample": a.steps},
           "us_per_step_median": {k: round(v, 1) for k, v in med.items()},
           "ema_minus_off_us": pairs("ema", "off"), "lerp_minus_off_us": pairs("lerp", "off"),
           "ema_minus_lerp_us": pairs("ema", "lerp"), "off2_minus_off_us": pairs("off2", "off"),
           "launch_us": adam_launch_times(vae.flat_params.numel(), dev),
           "samples_us": {k: [round(x, 1) for x in v] for k, v in samples.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
