#!/usr/bin/env python3
"""Time note splicing on a batch of songs (64 songs of 64 bars by default, a share `--p` of the cells active with 1..6 notes each,
the pieces of tools/bench_notes.py): `NoteBatch.windows(W, stride)` with W = 2 and stride 1, and `NoteBatch.join` of those
windows back into the songs (hop 1), against the host route a caller had before: `tolist()`, slicing the lists in Python (the
restatement of tests/splice_util.py) and `NoteBatch.from_lists`.  The device calls run with `check=False` and read nothing back:
a device-event pair on the stream and a host clock closed by a synchronise around each, warm-up, medians.  The kernel's share
is `ops.notes_splice` alone on segments built beforehand, events around `--inner` calls in a row.  Both device results are
compared with the host route's in the same run.  A missing GPU is an error.
Usage: python tools/bench_splice.py [B] [song_bars] [--W=2] [--stride=1] [--p=0.1] [--n=20] [--inner=20] [--host=2] [--json=FILE]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_notes import make_inputs, opt  # noqa: E402
from bench_stats import summary, timed  # noqa: E402
from polyphemus_amd import ops  # noqa: E402
from polyphemus_amd.generate import NoteBatch  # noqa: E402
from splice_util import join_np, windows_np  # noqa: E402


def host_clock(fn, n):
    out, v = None, []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) * 1e3)
    return out, summary(v)


def device_route(fn, n):
    for _ in range(3):
        fn()
    t = [timed(fn) for _ in range(n)]
    return {"device": summary([d for d, _ in t]), "host": summary([h for _, h in t])}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_splice: no GPU (nothing is measured without one)")
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    B = int(args[0]) if args else 64
    bars = int(args[1]) if len(args) > 1 else 64
    W, stride, p = opt("W", 2, int), opt("stride", 1, int), opt("p", 0.1, float)
    n, inner, n_host = opt("n", 20, int), opt("inner", 20, int), opt("host", 2, int)
    tokens, s, M = make_inputs(B, bars, p)
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, s)
    song = NoteBatch(notes[:M].contiguous(), track_ptr, totals, bars)   # (a notes buffer of M rows, not of the worst case)
    per = (bars - W) // stride + 1
    index = torch.arange(B * per, device="cuda").view(B, per)
    out = {"B": B, "song_bars": bars, "W": W, "stride": stride, "notes": M, "windows": B * per, "repeats": n, "inner": inner, "routes": {}}

    wins, _ = song.windows(W, stride=stride, check=False)
    out["window_notes"] = int(wins.totals[0])
    out["routes"]["windows"] = device_route(lambda: song.windows(W, stride=stride, check=False), n)
    joinable = stride <= W                                      # hop = stride puts the songs together again
    if joinable:
        out["routes"]["join"] = device_route(lambda: wins.join(index, hop_bars=stride, check=False), n)

    # the kernel's share: the three launches alone, on segments that are there already
    k = torch.arange(B * per, device="cuda")
    segments = torch.stack([k // per, (k % per) * stride, torch.zeros_like(k), torch.full_like(k, W)], 1).to(torch.int32)
    seg_ptr = torch.arange(B * per + 1, dtype=torch.int32, device="cuda")
    cap = song.notes.shape[0] * (-(-W // stride))

    def kernel():
        for _ in range(inner):
            ops.notes_splice(song.notes, song.track_ptr, bars, segments, seg_ptr, W, capacity=cap, check=False)
    kernel()
    out["routes"]["notes_splice alone (windows' segments)"] = summary([timed(kernel)[0] / inner for _ in range(n)])

    # the host route
    def host_windows():
        cut, _, _ = windows_np(song.tolist(), W, stride, total_bars=bars)
        return NoteBatch.from_lists(cut, W, device="cuda")
    want, out["routes"]["windows on the host: tolist + slicing + from_lists"] = host_clock(host_windows, n_host)
    Mw = int(want.totals[0])
    assert torch.equal(wins.track_ptr, want.track_ptr) and torch.equal(wins.notes[:Mw], want.notes) and torch.equal(wins.totals, want.totals)
    if joinable:
        def host_join():
            return NoteBatch.from_lists(join_np(wins.tolist(), index.tolist(), W, hop=stride), stride * (per - 1) + W, device="cuda")
        back, out["routes"]["join on the host: tolist + slicing + from_lists"] = host_clock(host_join, n_host)
        got = wins.join(index, hop_bars=stride)
        Mb = int(back.totals[0])
        assert torch.equal(got.track_ptr, back.track_ptr) and torch.equal(got.notes[:Mb], back.notes) and got.n_bars == back.n_bars
        assert torch.equal(got.track_ptr, song.track_ptr) and torch.equal(got.notes[:Mb], song.notes[:Mb])
    w, kshare = out["routes"]["windows"]["device"]["ms_median"], out["routes"]["notes_splice alone (windows' segments)"]["ms_median"]
    out["kernel_share_of_windows"] = round(kshare / w, 3) if w else None
    print(json.dumps(out, indent=1))
    path = opt("json", None, str)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
