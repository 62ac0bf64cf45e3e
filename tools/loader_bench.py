#!/usr/bin/env python3
"""What the data loaders deliver, and what a training loop fed by them runs at (the shape of BASELINE configs[1]: B = 256,
n_bars = 2, p = 0.25, max_notes = 4, d = 256, 8 layers).  `--samples` synthetic samples are written to a temporary directory as
the reference's `.npz` files, then:
  (a) batches/s of `DeviceLoader` with `num_workers` 0, 4 and 16 and a consumer that only waits for each batch;
  (b) the same for `ResidentLoader`, with and without transpose="random";
  (c) steps/s of `HipTrainer.train_step` fed by each loader and by one fixed batch; the fixed-batch loop is repeated
      `--repeats` times and its spread is the margin the resident-fed loop is judged against;
  (d) the one-off pack time (`ResidentDataset.from_dataset`) and `nbytes` of the store.
Every figure is a host clock around work that ends in a device synchronise, after a warm-up epoch, over whole epochs; medians
and the spread over `--repeats` runs.  The reader pool never has more than 16 threads.  A missing GPU is an error.
Usage: python tools/loader_bench.py [--samples=4096] [--batch=256] [--repeats=5] [--steps=32] [--d=256] [--layers=8] [--json=FILE]"""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polyphemus_amd.data import DeviceLoader, PolyphemusDataset, ResidentDataset, ResidentLoader  # noqa: E402
from polyphemus_amd.model import VAE  # noqa: E402
from polyphemus_amd.synthetic import disk_sample  # noqa: E402
from polyphemus_amd.trainer import HipTrainer  # noqa: E402

DEV = "cuda"


def opt(name, default, kind):
    for a in sys.argv[1:]:
        if a.startswith(f"--{name}="):
            return kind(a.split("=", 1)[1])
    return default


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2), "runs": len(v)}


def batches_per_s(loader, repeats):
    """a consumer that only waits for each batch; the first epoch is the warm-up"""
    rates = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = 0
        for batch in loader:
            torch.cuda.current_stream().synchronize()
            count += 1
        dt = time.perf_counter() - t0
        if r:
            rates.append(count / dt)
    return spread(rates)


def steps_per_s(trainer, feed, steps, repeats):
    """`feed()` yields the batches of one run of `steps` steps; the first run is the warm-up"""
    rates = []
    for r in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = 0
        for batch in feed():
            trainer.train_step(batch)
            count += 1
            if count == steps:
                break
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r:
            rates.append(count / dt)
    return spread(rates)


def epochs(loader):
    def feed():
        while True:
            yield from loader
    return feed


def main():
    if not torch.cuda.is_available():
        raise SystemExit("loader_bench: no GPU (nothing is measured without one)")
    n, B, repeats, steps = opt("samples", 4096, int), opt("batch", 256, int), opt("repeats", 5, int), opt("steps", 32, int)
    d, layers, nb = opt("d", 256, int), opt("layers", 8, int), 2
    out = {"samples": n, "batch": B, "n_bars": nb, "p": 0.25, "max_notes": 4, "d": d, "layers": layers, "repeats": repeats,
           "steps_per_run": steps}
    with tempfile.TemporaryDirectory() as tmp:
        rng = np.random.default_rng(1234)
        for i in range(n):
            c, s = disk_sample(rng, nb, 0.25, 4)
            np.savez(os.path.join(tmp, f"{i:06d}.npz"), c_tensor=c, s_tensor=s)
        ds = PolyphemusDataset(tmp, nb)

        # (d) the one-off cost of the store
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        resident = ResidentDataset.from_dataset(ds, device=DEV, num_workers=16)
        torch.cuda.synchronize()
        out["pack"] = {"seconds_16_readers": round(time.perf_counter() - t0, 3), "nbytes": resident.nbytes,
                       "bytes_per_sample": round(resident.nbytes / n, 1), "rows": int(resident.rows.shape[0])}

        # (a), (b): what the loaders deliver to a consumer that only waits
        rate = out["batches_per_s"] = {}
        for workers in (0, 4, 16):
            rate[f"DeviceLoader num_workers={workers}"] = batches_per_s(DeviceLoader(ds, B, shuffle=True, device=DEV, num_workers=workers), repeats)
        rate["ResidentLoader"] = batches_per_s(ResidentLoader(resident, B, shuffle=True), repeats)
        rate["ResidentLoader transpose=random"] = batches_per_s(ResidentLoader(resident, B, shuffle=True, transpose="random"), repeats)

        # (c): the training loop
        cfg = dict(dropout=0, batch_norm=True, gnn_n_layers=layers, d=d, n_bars=nb, resolution=8)
        torch.manual_seed(0)
        vae = VAE(**cfg, device=DEV).to(DEV)
        vae.train()
        trainer = HipTrainer(vae, lr=0.0, betas=(0.9, 0.98), eps=1e-9)      # (rate 0: every step starts from the same parameters)
        fixed = resident.batch(np.arange(B))
        run = out["steps_per_s"] = {}
        run["one fixed batch"] = steps_per_s(trainer, lambda: iter([fixed] * steps), steps, repeats)
        run["ResidentLoader"] = steps_per_s(trainer, epochs(ResidentLoader(resident, B, shuffle=True)), steps, repeats)
        run["ResidentLoader transpose=random"] = steps_per_s(trainer, epochs(ResidentLoader(resident, B, shuffle=True, transpose="random")),
                                                             steps, repeats)
        for workers in (0, 16):
            run[f"DeviceLoader num_workers={workers}"] = steps_per_s(
                trainer, epochs(DeviceLoader(ds, B, shuffle=True, device=DEV, num_workers=workers)), steps, repeats)
        run["one fixed batch, again"] = steps_per_s(trainer, lambda: iter([fixed] * steps), steps, repeats)
    f, r = run["one fixed batch"], run["ResidentLoader"]
    out["verdict"] = {"fixed_batch_spread_steps_per_s": round(f["max"] - f["min"], 2),
                      "resident_minus_fixed_median": round(r["median"] - f["median"], 2),
                      "resident_slower_than_the_margin": bool(f["median"] - r["median"] > f["max"] - f["min"])}
    print(json.dumps(out, indent=1))
    path = opt("json", None, str)
    if path:
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
