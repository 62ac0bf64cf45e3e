#!/usr/bin/env python3
"""Time the way from note events to the encoder's batch at the generation workload of DESIGN §5 (B = 256 two-bar pieces,
G = 512 bars; the pieces are those of tools/bench_notes.py, as `ops.notes_from_tokens` writes them): `ops.tokens_from_notes`
alone, `graphs.device_batch_from_notes` (the same plus `ops.graph_build`), and beside them `device_batch_from_structure` with a
dense token grid that already lies on the device.  A host clock around every call (each ends in a host read, so the clock covers
finished work); warm-up, medians.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times come out of the same run.
A missing GPU is an error.
Usage: python tools/bench_notes_in.py [B] [n_bars] [--p=0.25] [--n=20] [--json=FILE]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_notes import make_inputs, opt  # noqa: E402
from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.graphs import device_batch_from_notes, device_batch_from_structure  # noqa: E402


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_notes_in: no GPU (nothing is measured without one)")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    p, n = opt("p", 0.25, float), opt("n", 20, int)
    tokens, s, M = make_inputs(B, nb, p)
    notes, track_ptr, _ = ops.notes_from_tokens(tokens, s)
    notes = notes[:M].contiguous()
    s_f, tok, info = ops.tokens_from_notes(notes, track_ptr, nb)
    N = info["num_nodes"]
    assert N == tokens.shape[0] and info["dropped"] == 0 and torch.equal(s_f.view(s.shape).bool(), s)
    assert torch.equal(tok[:, 1:, 0], tokens[..., 0])
    grid = torch.zeros(B * nb, 4, 32, 16, 2, dtype=torch.int32, device="cuda")
    grid[s.view(-1, 4, 32)] = tok
    routes = {"tokens_from_notes": lambda: ops.tokens_from_notes(notes, track_ptr, nb),
              "device_batch_from_notes": lambda: device_batch_from_notes(notes, track_ptr, nb),
              "device_batch_from_structure + token grid": lambda: device_batch_from_structure(s_f, nb, token_grid=grid)}
    for fn in routes.values():
        for _ in range(3):
            fn()
    whole = {k: [] for k in routes}
    for _ in range(n):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            whole[k].append((time.perf_counter() - t0) * 1e3)
    out = {"B": B, "n_bars": nb, "bars": B * nb, "nodes": N, "notes": M, "note_bytes": 12 * M, "node_bytes": 128 * N,
           "token_grid_bytes": grid.numel() * 4, "repeats": n, "routes": {}}
    for k in routes:
        out["routes"][k] = {"ms_median": round(statistics.median(whole[k]), 4), "ms_min": round(min(whole[k]), 4),
                            "ms_max": round(max(whole[k]), 4)}
        r = out["routes"][k]
        print(f"{k:45s} B={B} n_bars={nb} N={N} M={M}: {r['ms_median']:8.4f} ms (min {r['ms_min']:.4f}, max {r['ms_max']:.4f})")
    print(json.dumps(out))
    path = opt("json", None, str)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
