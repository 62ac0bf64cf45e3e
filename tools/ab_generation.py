#!/usr/bin/env python3
"""Bit identity of the generation entry points between two builds of the library.

    PM_LIB_PATH=/path/to/libpolyphemus_hip.so python tools/ab_generation.py run OUT.npz
    python tools/ab_generation.py compare A.npz B.npz

`run` makes a fixed set of calls (inputs from seeded CPU generators, so two processes see the same bytes) under the library
this process loaded and writes every output array to OUT.npz; one process per library, since PM_LIB_PATH is read at import.
`compare` holds two such files against each other byte for byte and exits 1 on the first kind of difference it finds."""
import os
import sys

import numpy as np


def structures(G, gen):
    """{name: bool [1,G,4,32]}: a random structure with empty bars, and the all-zero one"""
    import torch
    s = torch.rand(1, G, 4, 32, generator=gen) < 0.1
    s[:, ::3] = False
    if G == 1:
        s[0, 0, 2, 5] = True
    return {"random": s, "zeros": torch.zeros(1, G, 4, 32, dtype=torch.bool)}


def logits_sets(N, gen):
    import torch
    out = {}
    for name, x in (("scale1", torch.randn(N, 15, 230, generator=gen)), ("scale3", torch.randn(N, 15, 230, generator=gen) * 3),
                    ("grid", (torch.randn(N, 15, 230, generator=gen) * 2).round() / 2)):
        x[0, 0, :] = float("nan")                                   # rows of non-finite logits, whole and in part
        x[0, 1, :] = float("-inf")
        x[0, 2, ::7] = float("inf")
        x[0, 3, 5] = float("nan")
        x[0, 4, 1:] = float("-inf")
        x[0, 4, 0] = float("nan")
        x[-1, 14, 128:140] = float("-inf")
        out[name] = x
    return out


def run(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polyphemus_amd import ops
    from polyphemus_amd._lib import LIB_PATH
    gen = torch.Generator().manual_seed(20261020)
    out = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            out[f"{name}/{i}"] = t.detach().cpu().numpy()

    for G in (1, 7, 9, 300, 1025):
        for sname, s in structures(G, gen).items():
            tag = f"G{G}/{sname}"
            sd = s.cuda()
            N = int(s.sum())
            g = ops.graph_build(sd.float(), 1)                       # (switches cell [0,0] of the empty bars on in its own copy)
            put(f"graph_build/{tag}", *[g[k] for k in ("edge_index", "edge_type", "edge_dist", "bars", "batch", "is_drum", "node_cell",
                                                       "node_ptr", "edge_ptr")])
            put(f"node_tracks/{tag}", ops.node_tracks(sd, N), ops.node_tracks(sd, N + 3, check=False))
            tok = torch.randint(0, 131, (N, 15, 2), generator=gen, dtype=torch.int32)
            tok[..., 1] %= 99
            tok[:, 4:, 0][torch.rand(N, 11, generator=gen) < 0.3] = 129
            notes, track_ptr, totals = ops.notes_from_tokens(tok.cuda(), sd)
            put(f"notes_from_tokens/{tag}", notes[:int(totals[0])], track_ptr, totals)
            if G <= 9:
                c = torch.randn(N, 15, 230, generator=gen)
                put(f"mtp_from_logits/{tag}", ops.mtp_from_logits(c.cuda(), sd))
                put(f"mtp_from_tokens/{tag}", ops.mtp_from_tokens(tok.cuda(), sd))
        x = (torch.randn(1, G, 4, 32, generator=gen) * 3 - 2).cuda()
        put(f"binary_from_logits/G{G}", ops.binary_from_logits(x), ops.binary_from_logits(x, 0.3))
        grid = np.zeros((4, 32), dtype=bool)
        grid[0], grid[1, ::2], grid[2], grid[3, ::4] = True, True, True, True
        for rname, kw in (("no_noise", dict(temperature=0.0)), ("noise", dict(temperature=1.0, seed=1)),
                          ("ranks", dict(temperature=1.0, min_active=1, max_active=12, seed=1)),
                          ("grids", dict(temperature=1.0, min_active=1, max_active=8, seed=1, allowed_steps=grid, return_counts=True))):
            r = ops.sample_structure(x, **kw)
            put(f"sample_structure/G{G}/{rname}", *(r if isinstance(r, tuple) else (r,)))

    routes = {"greedy": dict(temperature=0.0), "plain": dict(), "top_k5": dict(top_k=5), "top_k40": dict(top_k=40),
              "top_p": dict(top_p=0.9), "both": dict(top_k=40, top_p=0.9), "T0.5_top_k1": dict(temperature=0.5, top_k=1)}
    mask = torch.rand(4, 128, generator=gen) < 0.5
    chord_extra = {"T01": dict(temperature=(0.0, 1.0)), "T10": dict(temperature=(1.0, 0.0)), "mask": dict(allowed_pitches=mask),
                   "mask_top_k5": dict(allowed_pitches=mask, top_k=5), "min0_max1": dict(min_notes=0, max_notes=1),
                   "T01_both": dict(temperature=(0.0, 1.0), top_k=40, top_p=0.9)}
    for N in (1, 5, 273):
        track = torch.randint(0, 4, (N,), generator=gen, dtype=torch.uint8).cuda()
        for lname, x in logits_sets(N, gen).items():
            xd = x.cuda()
            for rname, kw in routes.items():
                put(f"sample_tokens/N{N}/{lname}/{rname}", ops.sample_tokens(xd, seed=7, **kw))
                put(f"sample_chords/N{N}/{lname}/{rname}", *ops.sample_chords(xd, track, seed=7, **kw))
            for rname, kw in chord_extra.items():
                put(f"sample_chords/N{N}/{lname}/{rname}", *ops.sample_chords(xd, track, seed=7, **kw))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes from {LIB_PATH} -> {path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    if sorted(a.files) != sorted(b.files):
        print("different sets of arrays:", sorted(set(a.files) ^ set(b.files))[:10])
        return 1
    bad = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    for k in bad[:20]:
        print("differs:", k, a[k].dtype, a[k].shape, b[k].shape)
    print(f"{len(a.files)} arrays, {sum(a[k].nbytes for k in a.files)} bytes: {'ALL IDENTICAL' if not bad else f'{len(bad)} DIFFER'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
