"""numpy restatement of what the reference's `muspy_from_mtp` (utils.py:83-124) reads out of a piece, from the tokens: the
yardstick of the note-event tests.  tests/test_notes_golden.py ties it to notes recorded from the reference itself."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"lmd2_tiny": (8, 2), "nb3_tiny": (6, 3)}                  # case: (B, n_bars)


def notes_ref(tokens, s_tensor):
    """tokens int [N,15,2] (pitch, duration), s_tensor [B,n_bars,4,32] -> (notes int32 [M,3], track_ptr int32 [4B+1]).  Nodes
    are the active cells in (piece, bar, track, step) order; a cell whose node index is >= N is silent.  Per piece and track
    the reference walks the time t = 32 bar + step, then the 15 slots: break at pitch 129 / 130 or duration 97 / 98, skip
    pitch 128 (and never a duration 96: utils.py:114-115), else the note (t, pitch, min(duration + 1, 32 n_bars - t)).  A
    token outside its head's range reads as 0 (the arg-max of an all-zero head)."""
    tokens, s = np.asarray(tokens).astype(np.int64), np.asarray(s_tensor) != 0
    B, n_bars = s.shape[:2]
    N = tokens.shape[0]
    pitch = np.where((tokens[..., 0] >= 0) & (tokens[..., 0] < 131), tokens[..., 0], 0)
    dur = np.where((tokens[..., 1] >= 0) & (tokens[..., 1] < 99), tokens[..., 1], 0)
    node = np.cumsum(s.reshape(-1)).reshape(s.shape) - 1             # node index of an active cell
    rows, track_ptr = [], [0]
    for i in range(B):
        for k in range(4):
            for t in range(32 * n_bars):
                b, step = divmod(t, 32)
                n = int(node[i, b, k, step])
                if not s[i, b, k, step] or n >= N:
                    continue
                for j in range(15):
                    p, d = int(pitch[n, j]), int(dur[n, j])
                    if p in (129, 130) or d in (97, 98):
                        break
                    if p == 128:
                        continue
                    rows.append((t, p, min(d + 1, 32 * n_bars - t)))
            track_ptr.append(len(rows))
    return np.asarray(rows, np.int32).reshape(-1, 3), np.asarray(track_ptr, np.int32)


def as_lists(notes, track_ptr):
    """per piece, four lists of (time, pitch, duration) tuples: the form of `NoteBatch.tolist()`"""
    notes, ptr = np.asarray(notes).tolist(), np.asarray(track_ptr).tolist()
    return [[[tuple(r) for r in notes[ptr[4 * i + k]:ptr[4 * i + k + 1]]] for k in range(4)] for i in range((len(ptr) - 1) // 4)]


def looped_ref(pieces, n_loops, n_bars, resolution=8):
    """`loop_muspy_music` (utils.py:144-160) on such lists: for i = 1 .. n_loops - 1, for every track, every note of the
    ORIGINAL track again at time + i * n_bars * 4 * resolution, appended behind what the track holds by then."""
    out = [[list(track) for track in piece] for piece in pieces]
    for p, piece in enumerate(pieces):
        for i in range(1, n_loops):
            for k, track in enumerate(piece):
                for (t, pitch, d) in track:
                    out[p][k].append((t + i * n_bars * 4 * resolution, pitch, d))
    return out


def load_case_tokens(name):
    """(arg-max tokens int32 [N,15,2], s_tensor uint8 [B,n_bars,4,32], c_logits fp32 [N,15,230]) of a golden case"""
    B, n_bars = CASES[name]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    c = z["eval/c_logits"]
    tokens = np.stack([c[..., :131].argmax(-1), c[..., 131:].argmax(-1)], -1).astype(np.int32)
    return tokens, z["in/s_tensor"].reshape(B, n_bars, 4, 32), c


def load_notes(name):
    z = np.load(os.path.join(GOLDEN, f"{name}_notes.npz"), allow_pickle=False)
    return z["notes"], z["track_ptr"]
