"""numpy restatement of the two infill kernels (csrc/infill.hip), written from the rules of "Infill" in
include/polyphemus_hip.h: the yardstick of the infill tests.  Node numbers come from `np.flatnonzero` in cell order."""
import numpy as np

EOS, PAD = (129, 97), (130, 98)


def infill_ref(s_in, tokens_in, s_model, tokens_drawn, region):
    """s_in [G,4,32] 0/1, tokens_in int [N_in,16,2], s_model [G,4,32] 0 / non-zero, tokens_drawn int [N,15,2] (the drawn
    tokens of the first N nodes of the merged structure), region [R,4,32] or [B,n_bars,4,32] with R = G or a divisor of G
    (bar g reads row g % R) -> (s_out bool [G,4,32], bar_forced int32 [G], tokens int32 [N,15,2], status int32 [5]).
      structure : a cell is on iff (region ? s_model : s_in); a bar without a cell gets [0,0] and bar_forced = 1.
      tokens    : a node of s_out inside the region keeps its drawn row; one outside takes tokens_in[n_in, 1:] of the input's
                  node of the same cell, or, where that cell is off in s_in or n_in >= N_in, (EOS, EOS) then (PAD, PAD).
      status    : cells of s_out, cells of s_in, kept nodes (below N), kept nodes without a source, bars forced."""
    a = np.asarray(s_in).reshape(-1, 4, 32) != 0
    m = np.asarray(s_model).reshape(-1, 4, 32) != 0
    r = np.asarray(region).reshape(-1, 4, 32) != 0
    G, R = len(a), len(r)
    assert m.shape == a.shape and R >= 1 and G % R == 0
    r = r[np.arange(G) % R]
    out = np.where(r, m, a)
    forced = ~out.any(axis=(1, 2))
    out[forced, 0, 0] = True
    tokens_in = np.asarray(tokens_in).reshape(-1, 16, 2)
    tokens = np.array(tokens_drawn, np.int32).reshape(-1, 15, 2)
    N, N_in = len(tokens), len(tokens_in)
    cells_out, cells_in = np.flatnonzero(out.reshape(-1)), np.flatnonzero(a.reshape(-1))
    node_in = np.full(a.size, N_in, np.int64)
    node_in[cells_in] = np.arange(len(cells_in))
    kept = lost = 0
    for n, c in enumerate(cells_out[:N]):
        if r.reshape(-1)[c]:
            continue
        kept += 1
        if node_in[c] < N_in:
            tokens[n] = tokens_in[node_in[c], 1:]
        else:
            lost += 1
            tokens[n, 0], tokens[n, 1:] = EOS, PAD
    status = np.asarray([len(cells_out), len(cells_in), kept, lost, int(forced.sum())], np.int32)
    return out, forced.astype(np.int32), tokens, status
