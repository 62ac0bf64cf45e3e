#!/usr/bin/env python3
"""Time sampled generation (csrc/sample.hip, k_mtp_fill<true>) at the generation workload of DESIGN §5 (B = 256, two bars):
`k_sample_tokens` on its greedy, unfiltered, top-k and top-p routes with its bytes over time against the 8 TB/s roof,
`k_sample_chords` (chord-aware sampling) on the same routes beside it in the same run, on the same logits (chords that run to
max_notes) and on logits with the EOS column raised (chords that end early), `node_tracks`,
`mtp_from_tokens` against `mtp_from_logits`, and `generate_music` sampled against `generate_music` without sampling
arguments (the call as it was), alternated in one process.  Device events around every call, medians.
Usage: python tools/bench_sampling.py [B] [n_bars] [--json=FILE]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.generate import ChordRules, generate_music  # noqa: E402

ROOF = 8.0e12           # HBM3E bytes/s


def times(fns, n=30, warm=3):
    """{name: [us per call]}: the calls alternate, one device-event pair around each; every call starts on an idle device (a call
    that ends without a synchronise would otherwise hide the launch latency of the one behind it)"""
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
    B = int(args[0]) if args else 256
    nb = int(args[1]) if len(args) > 1 else 2
    out = {"B": B, "n_bars": nb}
    torch.manual_seed(0)
    s = (torch.rand(B, nb, 4, 32, device="cuda") < 0.25)
    s[:, :, 0, 0] |= ~s.any(-1).any(-1)
    N = int(s.sum())
    c = torch.randn(N, 15, 230, device="cuda") * 3
    rows, byts = N * 15, N * 15 * (230 * 4 + 8)
    out.update(nodes=N, rows=rows, sample_bytes=byts)
    routes = {"greedy (temperature 0)": dict(temperature=0.0), "unfiltered": dict(), "top_k=40": dict(top_k=40),
              "top_p=0.9": dict(top_p=0.9), "top_k=40, top_p=0.9": dict(top_k=40, top_p=0.9)}
    ts = times({k: (lambda kw=kw: ops.sample_tokens(c, seed=1, **kw)) for k, kw in routes.items()})
    out["k_sample_tokens"] = {}
    for k, v in ts.items():
        r = summary(v)
        r["TB_per_s"] = round(byts / r["median_us"] / 1e6, 3)
        r["share_of_roof"] = round(byts / (r["median_us"] * 1e-6) / ROOF, 3)
        out["k_sample_tokens"][k] = r
        print(f"sample_tokens {k:24s} rows={rows}: {r['median_us']:8.1f} us (min {r['min_us']:.1f})  {r['TB_per_s']:6.3f} TB/s "
              f"= {100 * r['share_of_roof']:.1f} % of the roof ({byts / 1e6:.0f} MB)")
    # chord-aware sampling beside it: the same logits (an EOS is one of 129 candidates: nearly every chord runs to max_notes =
    # 14, all 15 rows read), and the EOS column raised by 6 (= 2 sigma, as in tests/test_chords_gpu.py: chords end early and the
    # rows behind the end are not read).  Default rules: min_notes 1, max_notes 14, every pitch allowed.
    track = ops.node_tracks(s, N)
    c_eos = c.clone()
    c_eos[:, :, 129] += 6.0
    out["k_sample_chords"] = {}
    for label, logits in (("chords run to max_notes", c), ("EOS raised by 6", c_eos)):
        notes = float(ops.sample_chords(logits, track, seed=1)[1].float().mean())
        calls = {}
        for k, kw in routes.items():
            calls[f"tokens {k}"] = lambda kw=kw, logits=logits: ops.sample_tokens(logits, seed=1, **kw)
            calls[f"chords {k}"] = lambda kw=kw, logits=logits: ops.sample_chords(logits, track, seed=1, **kw)
        ts = times(calls)
        out["k_sample_chords"][label] = {"mean_notes_unfiltered": round(notes, 2), **{k: summary(v) for k, v in ts.items()}}
        for k in routes:
            a, b = summary(ts[f"tokens {k}"]), summary(ts[f"chords {k}"])
            print(f"sample_chords [{label}, {notes:.2f} notes per node] {k:24s} N={N}: {b['median_us']:8.1f} us (min {b['min_us']:.1f}) "
                  f"against sample_tokens {a['median_us']:8.1f} us (min {a['min_us']:.1f})")
    ts = times({"node_tracks": lambda: ops.node_tracks(s, N, check=False)})
    out["node_tracks"] = summary(ts["node_tracks"])
    print(f"node_tracks      N={N}: {out['node_tracks']['median_us']:8.1f} us (min {out['node_tracks']['min_us']:.1f})")
    tok = ops.sample_tokens(c, seed=1)
    sf = s.float()
    ts = times({"mtp_from_logits": lambda: ops.mtp_from_logits(c, sf, check=False),
                "mtp_from_tokens": lambda: ops.mtp_from_tokens(tok, sf, check=False)})
    out["mtp"] = {k: summary(v) for k, v in ts.items()}
    for k, v in out["mtp"].items():
        print(f"{k:16s} N={N}: {v['median_us']:8.1f} us (min {v['min_us']:.1f}); writes {s.numel() * 13800 / 1e6:.0f} MB")

    # generate_music on the model of bench.py's generation workload.  Untrained, its own thresholded structure has one forced
    # cell per bar (N = B * n_bars): the call is then the decoder and the silence write.  The structure `s` above (p = 0.25,
    # N as in the kernel timings) enters as structure conditioning.
    from polyphemus_amd.model import VAE
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=8, d=256, n_bars=nb, resolution=8, device="cuda").to("cuda")
    vae.eval()
    z = torch.randn(B, 256, device="cuda")
    out["generate_music"] = {}
    with torch.no_grad():
        graph = vae.decoder._structure_from_binary(s)
        for label, cond in (("own structure", ()), ("structure of p = 0.25", (graph, s))):
            calls = {"as it was (logits)": lambda: generate_music(vae, z, *cond),
                     "sampled, temperature=1": lambda: generate_music(vae, z, *cond, temperature=1.0, seed=3),
                     "sampled, top_k=40": lambda: generate_music(vae, z, *cond, top_k=40, seed=3),
                     "sampled, top_k=40 top_p=0.9": lambda: generate_music(vae, z, *cond, top_k=40, top_p=0.9, seed=3),
                     "chords, temperature=1": lambda: generate_music(vae, z, *cond, seed=3, chord_rules=ChordRules()),
                     "chords, top_k=40 top_p=0.9": lambda: generate_music(vae, z, *cond, top_k=40, top_p=0.9, seed=3,
                                                                          chord_rules=ChordRules()),
                     "decoder alone": lambda: vae.decoder(z, cond[0] if cond else None)}
            nodes = int(generate_music(vae, z, *cond, return_tokens=True)[2].shape[0])
            ts = times(calls, n=15)
            out["generate_music"][label] = {"nodes": nodes, **{k: summary(v) for k, v in ts.items()}}
            for k, v in ts.items():
                r = summary(v)
                print(f"generate_music [{label}, N={nodes}] {k:28s}: {r['median_us'] / 1e3:8.3f} ms (min {r['min_us'] / 1e3:.3f}, "
                      f"max {r['max_us'] / 1e3:.3f})")
    for a in sys.argv[1:]:
        if a.startswith("--json="):
            with open(a[7:], "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
