#!/usr/bin/env python3
"""Time the per-piece scores (`ops.score_tokens`, `ops.score_structure`; csrc/score.hip) at the BASELINE configs[1] sizes
(B = 256 two-bar pieces, a quarter of the cells active: N about 16 k nodes, logits [N,15,230] = 226 MB) next to the torch chain
they replace: `log_softmax` on both heads, a gather, the PAD masks and an `index_add` by a node -> (bar, track) map.  The map is
built once outside the timed region (the chain's best case: a caller has to rebuild it from `s_tensor`), and the chain gives
the log-probabilities only, not the hit counts.  Device events on the stream around `--inner` calls in a row, warm-up, medians;
`check=False`, so neither route reads anything back.  A missing GPU is an error.
Usage: python tools/bench_score.py [B] [n_bars] [--p=0.25] [--n=20] [--inner=20] [--json=FILE]"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_notes import make_inputs, opt  # noqa: E402
from polyphemus_amd import ops  # noqa: E402


def timed(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def summary(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_score: no GPU (nothing is measured without one)")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    p, n, inner = opt("p", 0.25, float), opt("n", 20, int), opt("inner", 20, int)
    tokens, s, _ = make_inputs(B, nb, p)
    N = tokens.shape[0]
    torch.manual_seed(0)
    c_logits = 3.0 * torch.randn(N, 15, 230, device="cuda")
    s_logits = 2.0 * torch.randn(B, nb, 4, 32, device="cuda")
    bar, cell = torch.nonzero(s.reshape(-1, 128), as_tuple=True)
    seg = bar * 4 + cell // 32                                                     # node -> (bar, track)
    tgt = tokens.long()

    def chain():
        out = torch.zeros(B * nb * 4, 2, device="cuda")
        for h, (lo, hi, pad) in enumerate(((0, 131, 130), (131, 230, 98))):
            on = tgt[..., h] != pad
            lp = F.log_softmax(c_logits[..., lo:hi], dim=-1).gather(-1, torch.where(on, tgt[..., h], 0)[..., None])[..., 0]
            out[:, h].index_add_(0, seg, (lp * on).sum(1))
        return out

    def chain_structure():
        return -F.binary_cross_entropy_with_logits(s_logits, s.float(), reduction="none").sum(-1)

    routes = {"score_tokens": lambda: ops.score_tokens(c_logits, tokens, s, check=False), "torch chain (tokens)": chain,
              "score_structure": lambda: ops.score_structure(s_logits, s), "torch chain (structure)": chain_structure}
    want, got = chain().view(B, nb, 4, 2).double(), ops.score_tokens(c_logits, tokens, s)[0]
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-3), float((got - want).abs().max())
    rows = int((tokens[..., 0] != 130).sum())
    out = {"B": B, "n_bars": nb, "nodes": N, "rows": 15 * N, "rows_with_a_target": rows, "logits_MB": round(N * 15 * 230 * 4 / 1e6, 1),
           "repeats": n, "inner": inner, "routes": {}}
    for fn in routes.values():
        timed(fn, 3)
    times = {k: [] for k in routes}
    for _ in range(n):
        for k, fn in routes.items():
            times[k].append(timed(fn, inner))
    for k, v in times.items():
        out["routes"][k] = summary(v)
    print(json.dumps(out, indent=1))
    path = opt("json", None, str)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
