#!/usr/bin/env python3
"""Time the two ways from drawn tokens to something a host can use, at the generation workload of DESIGN §5 (B = 256 two-bar
pieces, G = 512 bars): (a) the pianoroll route, `ops.mtp_from_tokens` plus the `.cpu()` copy of the pianoroll, which is where
the reference's `muspy_from_mtp` starts its host slot loop (that loop itself is not timed here: the reference is not
available where this runs); (b) `ops.notes_from_tokens` plus `NoteBatch.tolist()`, which ends with the notes as Python tuples
(and, between the two, the same call with only the `.cpu()` copy of its M rows, the like-for-like of (a)).
The routes alternate in one process on the same tokens; a device-event pair around the device part, a host clock around the
whole call (both end in a device-to-host copy, so the host clock covers finished work); warm-up, medians.  The device part of
each is also timed alone.  A missing GPU is an error.
Usage: python tools/bench_notes.py [B] [n_bars] [--p=0.25] [--n=20] [--json=FILE]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.generate import NoteBatch  # noqa: E402


def opt(name, default, cast):
    for a in sys.argv[1:]:
        if a.startswith(f"--{name}="):
            return cast(a.split("=", 1)[1])
    return default


def make_inputs(B, nb, p, seed=0):
    """a structure with a share p of the cells active, and chords as training data lays them out: 1..6 notes, one EOS, then PAD"""
    rng = np.random.default_rng(seed)
    s = rng.random((B, nb, 4, 32)) < p
    s[:, :, 0, 0] = True
    N = int(s.sum())
    tok = np.empty((N, 15, 2), np.int32)
    tok[..., 0], tok[..., 1] = 130, 98
    n_notes = rng.integers(1, 7, N)
    for j in range(6):
        on = n_notes > j
        tok[on, j, 0], tok[on, j, 1] = rng.integers(24, 96, int(on.sum())), rng.integers(0, 32, int(on.sum()))
    tok[np.arange(N), n_notes] = (129, 97)
    return torch.from_numpy(tok).cuda(), torch.from_numpy(s).cuda(), int(n_notes.sum())


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_notes: no GPU (nothing is measured without one)")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    p, n = opt("p", 0.25, float), opt("n", 20, int)
    tokens, s, M = make_inputs(B, nb, p)
    N = tokens.shape[0]

    def pianoroll():
        mtp = ops.mtp_from_tokens(tokens, s)
        return mtp, lambda: mtp.cpu()

    def notes():
        out = ops.notes_from_tokens(tokens, s)
        return out, lambda: NoteBatch(*out, nb).tolist()

    def notes_copy():
        out = ops.notes_from_tokens(tokens, s)
        return out, lambda: (out[0][:int(out[2][0])].cpu(), out[1].cpu())

    routes = {"pianoroll: mtp_from_tokens + .cpu()": pianoroll, "notes: notes_from_tokens + .cpu() of the M rows": notes_copy,
              "notes: notes_from_tokens + tolist()": notes}
    for fn in routes.values():
        for _ in range(3):
            fn()[1]()
    dev, whole = {k: [] for k in routes}, {k: [] for k in routes}
    for _ in range(n):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            _, to_host = fn()
            b.record()
            res = to_host()
            whole[k].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            dev[k].append(a.elapsed_time(b))
            del res
    assert sum(len(t) for piece in NoteBatch(*ops.notes_from_tokens(tokens, s), nb).tolist() for t in piece) == M
    out = {"B": B, "n_bars": nb, "bars": B * nb, "nodes": N, "notes": M, "pianoroll_bytes": B * nb * 128 * 15 * 230 * 4,
           "notes_bytes": 12 * M, "token_bytes": 120 * N, "repeats": n, "routes": {}}
    for k in routes:
        out["routes"][k] = {"device_part_ms_median": round(statistics.median(dev[k]), 4), "device_part_ms_min": round(min(dev[k]), 4),
                            "whole_ms_median": round(statistics.median(whole[k]), 3), "whole_ms_min": round(min(whole[k]), 3),
                            "whole_ms_max": round(max(whole[k]), 3)}
        r = out["routes"][k]
        print(f"{k:50s} B={B} n_bars={nb} N={N} M={M}: device part {r['device_part_ms_median']:9.4f} ms, to the host "
              f"{r['whole_ms_median']:9.3f} ms (min {r['whole_ms_min']:.3f}, max {r['whole_ms_max']:.3f})")
    print(json.dumps(out))
    path = opt("json", None, str)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
