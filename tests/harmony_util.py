"""numpy restatements of "Harmony" (include/polyphemus_hip.h: pm_note_chroma) and of what `NoteBatch.harmony` derives from the
chromagram, written as the plainest possible loops, and the hand-written chord sets the harmony tests compare with.
tests/test_harmony_abi.py ties them to hand-computed values; tests/test_harmony_gpu.py compares the device with them."""
import numpy as np

from stats_util import clamped_ranges

C_MAJOR, A_MINOR, C_MAJOR_SCALE, FREE = 0x091, 0x211, 0xAB5, 0xFFF
SETS = [C_MAJOR, A_MINOR, C_MAJOR_SCALE, FREE, 0x001, 0]
# the 24 triads in template order: major on C .. B, then minor on C .. B
TRIADS = [sum(1 << ((r + k) % 12) for k in iv) for iv in ((0, 4, 7), (0, 3, 7)) for r in range(12)]


def chroma_ref(notes, track_ptr, n_bars, seg_steps):
    """-> int32 [4B, 32 n_bars / seg_steps, 12]: a row counts iff 0 <= t < L = 32 n_bars, as the pitch clamp(p, 0, 127) of
    length clamp(d, 1, 96) sounding over [t, min(t + e, L)); every (note, step) pair adds one to its segment and class"""
    rows = np.asarray(notes).reshape(-1, 3).tolist()
    L = 32 * n_bars
    ranges = clamped_ranges(track_ptr, len(rows))
    out = np.zeros((len(ranges), L // seg_steps, 12), np.int32)
    for tr, (lo, hi) in enumerate(ranges):
        for (t, p, d) in rows[lo:hi]:
            if not 0 <= t < L:
                continue
            q, e = min(max(p, 0), 127), min(max(d, 1), 96)
            for s in range(t, min(t + e, L)):
                out[tr, s // seg_steps, q % 12] += 1
    return out


def sets_ref(chroma, tracks, snap=None):
    """chroma [B,4,S,12] -> the sets [B,S] of the pitch classes sounding in `tracks` (indices); with snap the best triad of
    every non-empty segment: weight inside minus weight outside, the lowest template index on ties"""
    B, _, S, _ = chroma.shape
    out = np.zeros((B, S), np.int64)
    for b in range(B):
        for s in range(S):
            w = [sum(int(chroma[b, k, s, c]) for k in tracks) for c in range(12)]
            bits = sum(1 << c for c in range(12) if w[c] > 0)
            if snap and bits:
                scores = [sum(w[c] if (t >> c) & 1 else -w[c] for c in range(12)) for t in TRIADS]
                bits = TRIADS[scores.index(max(scores))]
            out[b, s] = bits
    return out


def random_rows(rng, n, L):
    """n rows with times from -5 to L + 4, pitches from -6 to 139 and durations from -3 to 129: rows outside the piece, pitches
    and durations that are clamped, and notes that cross the piece's end are all among them for n of a few dozen"""
    return np.stack([rng.integers(-5, L + 5, n), rng.integers(-6, 140, n), rng.integers(-3, 130, n)], 1).astype(np.int32)
