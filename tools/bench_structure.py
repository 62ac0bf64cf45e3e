#!/usr/bin/env python3
"""Time structure sampling (csrc/sample.hip) at the generation workload of DESIGN §5 (B = 256, two bars, G = 512 bars):
`k_sample_structure` on its routes (no noise / noise, bounds that cannot bind / a rank pass on every track) beside
`k_binary_from_logits` on the same logits, and `generate_music(structure_rules=...)` against `generate_music` without the
keyword (the call as it was), alternated in one process.  Device events around every call, medians.
`--only-plain` times the keyword-less call alone (it also runs on a checkout that has no structure sampling).
`--trace=ROUTE` (no-noise | noise | ranks | grids) only launches `k_binary_from_logits` and that one route of
`k_sample_structure` 200 times each, for a kernel trace taken from outside (the kernels' own times, without the wrappers).
Usage: python tools/bench_structure.py [B] [n_bars] [--only-plain] [--trace=ROUTE] [--json=FILE]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.generate import generate_music  # noqa: E402
from polyphemus_amd.model import VAE  # noqa: E402


def times(fns, n=30, warm=3):
    """{name: [us per call]}: the calls alternate, one device-event pair around each, every call starts on an idle device"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    ev = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}


def summary(ts):
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1), "calls": len(ts)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    only_plain = "--only-plain" in sys.argv
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    out = {"B": B, "n_bars": nb, "bars": B * nb}
    torch.manual_seed(0)
    if not only_plain:
        from polyphemus_amd.generate import step_mask
        import numpy as np
        x = torch.randn(B, nb, 4, 32, device="cuda") * 3 - 2
        grid = np.stack([step_mask(), step_mask(2), step_mask(), step_mask(4)])
        trace = [a[8:] for a in sys.argv[1:] if a.startswith("--trace=")]
        if trace:
            route = {"no-noise": lambda: ops.sample_structure(x, 0.0), "noise": lambda: ops.sample_structure(x, 1.0, seed=1),
                     "ranks": lambda: ops.sample_structure(x, 1.0, min_active=1, max_active=12, seed=1),
                     "grids": lambda: ops.sample_structure(x, 1.0, min_active=1, max_active=8, seed=1, allowed_steps=grid,
                                                           return_counts=True)}[trace[0]]
            for _ in range(200):
                ops.binary_from_logits(x)
                route()
            torch.cuda.synchronize()
            return
        calls = {"binary_from_logits": lambda: ops.binary_from_logits(x),
                 "structure, no noise, bounds 0..32": lambda: ops.sample_structure(x, 0.0),
                 "structure, T=1, bounds 0..32": lambda: ops.sample_structure(x, 1.0, seed=1),
                 "structure, T=1, ranks on 4 tracks": lambda: ops.sample_structure(x, 1.0, min_active=1, max_active=12, seed=1),
                 "structure, T=1, ranks, grids, counts": lambda: ops.sample_structure(x, 1.0, min_active=1, max_active=8, seed=1,
                                                                                      allowed_steps=grid, return_counts=True),
                 "torch.empty alone": lambda: torch.empty(x.shape, dtype=torch.uint8, device="cuda")}
        ts = times(calls, n=50)
        out["kernels"] = {k: summary(v) for k, v in ts.items()}
        for k, v in out["kernels"].items():
            print(f"{k:40s} G={B * nb}: {v['median_us']:8.1f} us (min {v['min_us']:.1f}, max {v['max_us']:.1f})")

    # generate_music on the model of bench.py's generation workload.  Untrained, every structure logit is negative: the thresholded
    # structure has one forced cell per bar (N = B * n_bars), and so has the structure drawn without noise (its best cell
    # instead of [0,0]): the same work behind one different launch.  At temperature 1 about half the cells are drawn, and the
    # decoder and the pianoroll then work on that many more nodes.
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=8, d=256, n_bars=nb, resolution=8, device="cuda").to("cuda")
    vae.eval()
    z = torch.randn(B, 256, device="cuda")
    with torch.no_grad():
        calls = {"as it was (thresholded)": lambda: generate_music(vae, z)}
        if not only_plain:
            from polyphemus_amd.generate import StructureRules
            calls["as it was (thresholded), again"] = lambda: generate_music(vae, z)
            calls["structure_rules, no noise"] = lambda: generate_music(vae, z, structure_rules=StructureRules(temperature=0), seed=3)
            calls["structure_rules, T=1, at most 1 cell per track"] = lambda: generate_music(
                vae, z, structure_rules=StructureRules(max_active=1), seed=3)
            calls["structure_rules, defaults (T=1)"] = lambda: generate_music(vae, z, structure_rules=StructureRules(), seed=3)
        nodes = {k: int(fn()[1].sum()) for k, fn in calls.items()}
        ts = times(calls, n=15)
        out["generate_music"] = {k: {"nodes": nodes[k], **summary(v)} for k, v in ts.items()}
        for k, r in out["generate_music"].items():
            print(f"generate_music [N={r['nodes']}] {k:48s}: {r['median_us'] / 1e3:8.3f} ms (min {r['min_us'] / 1e3:.3f}, "
                  f"max {r['max_us'] / 1e3:.3f})")
    for a in sys.argv[1:]:
        if a.startswith("--json="):
            with open(a[7:], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
