"""numpy restatement of "Note statistics" (include/polyphemus_hip.h: pm_note_stats, pm_notes_select) and of the measures
`NoteStats` derives from the counts, written as the plainest possible loops: a per-step counter array per track, Python sets
for the distinct counts, float64 for the derived measures.  tests/test_stats_abi.py ties it to a hand-computed piece and to
the recorded reference notes of the golden cases; tests/test_stats_gpu.py compares the device with it."""
import math

import numpy as np

FIELDS = ("n_notes", "n_onsets", "pitch_min", "pitch_max", "n_pitches", "n_pitch_classes", "note_steps", "sounding_steps",
          "poly_steps", "max_polyphony", "max_chord", "out_of_range")
MAJOR = (0, 2, 4, 5, 7, 9, 11)


def clamped_ranges(track_ptr, M):
    """[(lo, hi)] per track with 0 <= lo <= hi <= M, whatever track_ptr holds (TrackRange of csrc/notes_in.hip)"""
    ptr = [int(v) for v in np.asarray(track_ptr).tolist()]
    out = []
    for tr in range(len(ptr) - 1):
        lo = min(max(ptr[tr], 0), M)
        out.append((lo, min(max(ptr[tr + 1], lo), M)))
    return out


def _word(bits):
    """32 booleans -> the int32 bit pattern (bit s = bits[s], bit 31 the sign)"""
    w = 0
    for s, b in enumerate(bits):
        if b:
            w |= 1 << s
    return w - (1 << 32) if w >= (1 << 31) else w


def stats_ref(notes, track_ptr, n_bars):
    """-> (track int32 [4B,12], pitch_class int32 [4B,12], onsets int32 [4B,n_bars], sounding int32 [4B,n_bars])"""
    notes = np.asarray(notes).reshape(-1, 3)
    rows = notes.tolist()
    L = 32 * n_bars
    ranges = clamped_ranges(track_ptr, len(rows))
    T = len(ranges)
    track, pcs = np.zeros((T, 12), np.int32), np.zeros((T, 12), np.int32)
    onsets, sounding = np.zeros((T, n_bars), np.int32), np.zeros((T, n_bars), np.int32)
    for tr, (lo, hi) in enumerate(ranges):
        sound, onset = [0] * L, [0] * L                      # notes sounding / starting at every step
        pitches, classes, pc = set(), set(), [0] * 12
        n = steps = outside = 0
        for (t, p, d) in rows[lo:hi]:
            if not 0 <= t < L:
                outside += 1
                continue
            q, e = min(max(p, 0), 127), min(max(d, 1), 96)
            end = min(t + e, L)
            n += 1
            steps += end - t
            pitches.add(q)
            classes.add(q % 12)
            pc[q % 12] += 1
            onset[t] += 1
            for s in range(t, end):
                sound[s] += 1
        track[tr] = (n, sum(1 for v in onset if v > 0), min(pitches) if pitches else 128, max(pitches) if pitches else -1,
                     len(pitches), len(classes), steps, sum(1 for v in sound if v > 0), sum(1 for v in sound if v > 1),
                     max(sound), max(onset), outside)
        pcs[tr] = pc
        for b in range(n_bars):
            onsets[tr, b] = _word([v > 0 for v in onset[32 * b:32 * b + 32]])
            sounding[tr, b] = _word([v > 0 for v in sound[32 * b:32 * b + 32]])
    return track, pcs, onsets, sounding


def derived_ref(track, pitch_class, onsets, sounding, n_bars, resolution=8):
    """the measures of `NoteStats` in float64: dict of [B,4] arrays, "empty_beat_rate" [B]"""
    T = len(track)
    B, L = T // 4, 32 * n_bars
    out = {k: np.zeros((B, 4)) for k in ("polyphony", "polyphony_rate", "pitch_class_entropy", "scale_consistency",
                                         "groove_consistency")}
    bits = lambda w: [(int(w) >> s) & 1 for s in range(32)]              # (Python's >> on a negative int keeps the pattern)
    for tr in range(T):
        i, k = divmod(tr, 4)
        rec = dict(zip(FIELDS, (int(v) for v in track[tr])))
        pc = [int(v) for v in pitch_class[tr]]
        n = sum(pc)
        out["polyphony"][i, k] = rec["note_steps"] / rec["sounding_steps"] if rec["sounding_steps"] else 0.0
        out["polyphony_rate"][i, k] = rec["poly_steps"] / L
        out["pitch_class_entropy"][i, k] = -sum(c / n * math.log2(c / n) for c in pc if c) if n else 0.0
        out["scale_consistency"][i, k] = max(sum(pc[(root + s) % 12] for s in MAJOR) for root in range(12)) / n if n else 0.0
        if n_bars == 1:
            out["groove_consistency"][i, k] = 1.0
        else:
            ham = [sum(a != b for a, b in zip(bits(onsets[tr, b]), bits(onsets[tr, b + 1]))) / 32 for b in range(n_bars - 1)]
            out["groove_consistency"][i, k] = 1.0 - sum(ham) / len(ham)
    assert 32 % resolution == 0
    empty = np.zeros(B)
    for i in range(B):
        beats = used = 0
        for b in range(n_bars):
            step = [any(bits(sounding[4 * i + k, b])[s] for k in range(4)) for s in range(32)]
            for beat in range(32 // resolution):
                beats += 1
                used += any(step[beat * resolution:(beat + 1) * resolution])
        empty[i] = 1.0 - used / beats
    out["empty_beat_rate"] = empty
    return out


def select_ref(notes, track_ptr, index):
    """-> (rows int32 [M',3], out_track_ptr int32 [4K+1], totals [M', cells], status [out of range, repeated])"""
    notes = np.asarray(notes).reshape(-1, 3)
    ranges = clamped_ranges(track_ptr, len(notes))
    B = len(ranges) // 4
    rows, ptr, cells, bad, rep, seen = [], [0], 0, 0, 0, set()
    for b in [int(v) for v in index]:
        if not 0 <= b < B:
            bad += 1
        elif b in seen:
            rep += 1
        else:
            seen.add(b)
            for k in range(4):
                lo, hi = ranges[4 * b + k]
                ptr.append(ptr[-1] + hi - lo)
                for i in range(lo, hi):
                    rows.append(tuple(int(v) for v in notes[i]))
                    cells += i == lo or notes[i, 0] != notes[i - 1, 0]
            continue
        ptr.extend([ptr[-1]] * 4)
    return (np.asarray(rows, np.int32).reshape(-1, 3), np.asarray(ptr, np.int32), [len(rows), int(cells)], [bad, rep])
