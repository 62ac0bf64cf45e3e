"""numpy / plain Python restatement of "Note splicing" (include/polyphemus_hip.h: pm_notes_splice) and of what
`NoteBatch.windows` / `NoteBatch.join` build on it, written as the plainest loops.  The silence filter and the transposition
restate the reference's preprocessing (preprocess.py:176-194 and 196-205) on an activity grid and on pitch tokens; of its
text only the one numpy expression whose accident the kernel has to reproduce is kept as it stands.  tests/test_splice_cpu.py ties all of it to cases computed by hand; tests/test_splice_gpu.py compares the device
with it."""
import numpy as np

from stats_util import clamped_ranges

MAX_PITCH_TOKEN = 127                                        # constants.py


def filter_ref(acts):
    """acts bool [4, n_bars] (track k has an onset in bar b) -> True iff the reference keeps the sequence"""
    acts = np.asarray(acts, bool)
    if acts.shape[1] == 1:                                   # one bar: dropped only if no track plays
        return bool(acts.any())
    # preprocess.py:182 as it stands: np.where walks the silent (track, bar) pairs in row-major order and [1] keeps their
    # bars, so a difference of 1 is two consecutive silent bars of a track, or the last silent bar of one track and the first
    # of the next track that has any
    if 1 in np.diff(np.where(acts == 0)[1]):
        return False
    return bool(acts.any(axis=0).all())                      # no bar in which every track is silent


def shift_ref(pitch, shift):
    """pitches of a track that is not the drums -> the pitch tokens the reference stores after its transposition: the token is
    the clamped pitch (preprocess.py:140), the shift is added and the sum clipped (preprocess.py:203-205)"""
    tok = np.asarray([max(min(int(p), MAX_PITCH_TOKEN), 0) for p in pitch], np.int64)
    tok = tok + int(shift)
    return np.clip(tok, a_min=0, a_max=MAX_PITCH_TOKEN)


def splice_ref(notes, track_ptr, src_bars, segments, seg_ptr, out_bars, shift=None, silence_rule=False):
    """-> (rows int32 [M',3], out_track_ptr int32 [4K+1], totals [M', cells], keep [K], status [not followed, bad seg_ptr
    entries]); the third status word is max(M' - capacity, 0), the caller's"""
    notes = np.asarray(notes).reshape(-1, 3)
    ranges = clamped_ranges(track_ptr, len(notes))
    B = len(ranges) // 4
    segments = [tuple(int(v) for v in s) for s in np.asarray(segments).reshape(-1, 4).tolist()]
    S = len(segments)
    sp = [int(v) for v in np.asarray(seg_ptr).tolist()]
    K = len(sp) - 1
    bad_ptr = sum(1 for e in range(K + 1) if sp[e] < 0 or sp[e] > S or (e > 0 and sp[e] < sp[e - 1]))
    rows, ptr, cells, bad_seg, keep = [], [0], 0, 0, []
    for j in range(K):
        lo = min(max(sp[j], 0), S)
        hi = min(max(sp[j + 1], lo), S)
        followed, end = [], 0
        for (p, sb, ob, nb) in segments[lo:hi]:
            if 0 <= p < B and nb >= 1 and sb >= 0 and sb + nb <= src_bars and ob >= end and ob + nb <= out_bars:
                followed.append((p, sb, ob, nb))
                end = ob + nb
            else:
                bad_seg += 1
        acts = np.zeros((4, out_bars), bool)
        for k in range(4):
            track = []
            for (p, sb, ob, nb) in followed:
                a, b = ranges[4 * p + k]
                for (t, pitch, d) in notes[a:b].tolist():
                    if 32 * sb <= t < 32 * (sb + nb):
                        track.append((t - 32 * sb + 32 * ob, pitch, d))
            if shift is not None and k > 0 and track:
                new = shift_ref([r[1] for r in track], shift[j])
                track = [(t, int(q), d) for (t, _, d), q in zip(track, new)]
            for i, r in enumerate(track):
                cells += i == 0 or r[0] != track[i - 1][0]
                acts[k, r[0] // 32] = True
            rows += track
            ptr.append(len(rows))
        keep.append(int(filter_ref(acts)) if silence_rule else 1)
    return (np.asarray(rows, np.int32).reshape(-1, 3), np.asarray(ptr, np.int32), [len(rows), int(cells)], keep, [bad_seg, bad_ptr])


def window_starts(song_bars, n_bars, stride):
    return list(range(0, song_bars - n_bars + 1, stride))


def windows_np(pieces, n_bars, stride=1, song_bars=None, total_bars=None):
    """the host route: `pieces` as `NoteBatch.tolist()` gives them -> (windows as such lists, song [K], start [K]); a window
    holds the notes whose onset lies in it, in list order, with the time counted from its first bar"""
    song_bars = [total_bars] * len(pieces) if song_bars is None else list(song_bars)
    out, song, start = [], [], []
    for b, piece in enumerate(pieces):
        for s in window_starts(song_bars[b], n_bars, stride):
            out.append([[(t - 32 * s, p, d) for (t, p, d) in track if 32 * s <= t < 32 * (s + n_bars)] for track in piece])
            song.append(b)
            start.append(s)
    return out, song, start


def window_acts(window, n_bars):
    acts = np.zeros((4, n_bars), bool)
    for k, track in enumerate(window):
        for (t, _, _) in track:
            acts[k, t // 32] = True
    return acts


def transposed(window, shift):
    """a window (four lists) with the tracks 1..3 shifted as the reference shifts their tokens"""
    return [list(window[0])] + [[(t, int(q), d) for (t, _, d), q in zip(track, shift_ref([r[1] for r in track], shift))]
                                for track in window[1:]]


def join_np(pieces, index, n_bars, hop=None):
    """pieces of `n_bars` bars as lists, index [K][G] (-1: silence) -> songs of hop (G - 1) + n_bars bars as lists: window g
    gives the notes of its first `hop` bars (all of them if it is the last) from bar g hop on"""
    hop = n_bars if hop is None else hop
    songs = []
    for row in index:
        song = [[], [], [], []]
        for g, i in enumerate(row):
            if i == -1:
                continue
            take = n_bars if g == len(row) - 1 else hop
            for k in range(4):
                song[k] += [(t + 32 * g * hop, p, d) for (t, p, d) in pieces[i][k] if t < 32 * take]
        songs.append(song)
    return songs
