#!/usr/bin/env python3
"""Time the harmony kernels at the generation workload of DESIGN §5 (B = 256, two bars, structure of p = 0.25) beside their
neighbours, alternated in one process: `sample_chords_at` (k_sample_chords<MODE, true>, a chart that binds Bass, Guitar and
Strings: a triad per bar; and a chart of 0xfff that binds all four tracks and so draws the very tokens of `sample_chords`: the
cost of the chart alone) against `sample_chords` on the same logits, rules and seed, on the routes and the two kinds of logits of
tools/bench_sampling.py; `node_cells` against `node_tracks`; `note_chroma` at 32, 8 and 1 steps per segment against
`note_stats` on the NoteBatch read from the sampled chords.  Device events around every call (the `times` of
tools/bench_sampling.py), medians, and the spread of `sample_chords` between the passes of the same run.
`--baseline` times only the entries that exist without the harmony kernels (`sample_chords`, `node_tracks`, `note_stats`), so
that the same file measures a checkout of the parent commit.
Usage: python tools/bench_harmony.py [B] [n_bars] [--passes=N] [--baseline] [--json=FILE]"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from bench_sampling import summary, times  # noqa: E402
from polyphemus_amd import ops  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opts = dict(a[2:].split("=", 1) if "=" in a else (a[2:], "1") for a in sys.argv[1:] if a.startswith("--"))
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    passes, baseline = int(opts.get("passes", 5)), "baseline" in opts
    out = {"B": B, "n_bars": nb, "baseline": baseline, "passes": passes}
    torch.manual_seed(0)
    s = (torch.rand(B, nb, 4, 32, device="cuda") < 0.25)
    s[:, :, 0, 0] |= ~s.any(-1).any(-1)
    N = int(s.sum())
    c = torch.randn(N, 15, 230, device="cuda") * 3
    c_eos = c.clone()
    c_eos[:, :, 129] += 6.0
    out["nodes"] = N
    track = ops.node_tracks(s, N)
    routes = {"unfiltered": dict(), "top_k=40, top_p=0.9": dict(top_k=40, top_p=0.9), "greedy (temperature 0)": dict(temperature=0.0)}
    if not baseline:
        from polyphemus_amd.generate import Harmony
        cells = ops.node_cells(s, N)
        triads = [0x091, 0x211, 0x221, 0x884]                                         # C, Am, F, G: one per bar
        chart = Harmony(np.asarray([triads[g % 4] for g in range(nb)]).reshape(nb, 1)).chart(B, nb, "cuda")
        free = torch.full_like(chart, 0xFFF)
    out["k_sample_chords"] = {}
    for label, logits in (("chords run to max_notes", c), ("EOS raised by 6", c_eos)):
        res = {}
        for k, kw in routes.items():
            per_pass = {"sample_chords": [], "sample_chords_at": [], "sample_chords_at, free chart": []}
            for _ in range(passes):
                calls = {"sample_chords": lambda kw=kw, logits=logits: ops.sample_chords(logits, track, seed=1, **kw)}
                if not baseline:
                    calls["sample_chords_at"] = lambda kw=kw, logits=logits: ops.sample_chords_at(logits, cells, chart, 0b1110, seed=1, **kw)
                    calls["sample_chords_at, free chart"] = lambda kw=kw, logits=logits: ops.sample_chords_at(logits, cells, free, 0b1111,
                                                                                                              seed=1, **kw)
                for name, v in times(calls).items():
                    per_pass[name].append(summary(v)["median_us"])
            res[k] = {name: {"pass_medians_us": v, "median_us": float(np.median(v)), "spread_us": round(max(v) - min(v), 1)}
                      for name, v in per_pass.items() if v}
            line = "  ".join(f"{name} {r['median_us']:8.1f} us (passes {r['pass_medians_us']})" for name, r in res[k].items())
            print(f"[{label}] {k:24s} N={N}: {line}")
        if not baseline:
            res["mean_notes"] = {"sample_chords": round(float(ops.sample_chords(logits, track, seed=1)[1].float().mean()), 2),
                                 "sample_chords_at": round(float(ops.sample_chords_at(logits, cells, chart, 0b1110, seed=1)[1].float().mean()), 2)}
            print(f"[{label}] mean notes per node: {res['mean_notes']}")
        out["k_sample_chords"][label] = res
    calls = {"node_tracks": lambda: ops.node_tracks(s, N, check=False)}
    if not baseline:
        calls["node_cells"] = lambda: ops.node_cells(s, N, check=False)
    out["node"] = {k: summary(v) for k, v in times(calls).items()}
    print("  ".join(f"{k} {v['median_us']:.1f} us (min {v['min_us']:.1f})" for k, v in out["node"].items()))
    # the NoteBatch of the sampled chords (EOS raised: a few notes per cell)
    tokens = ops.sample_chords(c_eos, track, seed=1)[0]
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, s)
    out["notes"] = int(totals[0])
    calls = {"note_stats": lambda: ops.note_stats(notes, track_ptr, nb)}
    if not baseline:
        for seg in (32, 8, 1):
            calls[f"note_chroma seg_steps={seg}"] = lambda seg=seg: ops.note_chroma(notes, track_ptr, nb, seg)
    out["stats"] = {k: summary(v) for k, v in times(calls).items()}
    print(f"M = {out['notes']} notes, B = {B}: " + "  ".join(f"{k} {v['median_us']:.1f} us (min {v['min_us']:.1f})" for k, v in out["stats"].items()))
    if "json" in opts:
        with open(opts["json"], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
