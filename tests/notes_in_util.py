"""numpy restatement of what the reference does to the notes of a piece before its encoder sees them (preprocess.py:118-157:
the per-track slot filling; data.py:148-153: cell [0,0] of an empty bar), over `NoteBatch`-layout arrays: the yardstick of the
notes-in tests.  tests/test_notes_in_abi.py ties it to the golden cases through `notes_util.notes_ref`."""
import numpy as np

from notes_util import notes_ref  # noqa: F401  (re-exported: the tests go there and back)

SOS, EOS, PAD = (128, 96), (129, 97), (130, 98)


def tokens_ref(notes, track_ptr, n_bars):
    """notes int [M,3] (time, pitch, duration), track_ptr int [4B+1] -> (s_tensor float32 [B n_bars,4,32], tokens int32
    [N,16,2], dropped).  Per (piece, track) the reference's loop: a counter per timestep that starts at 1; a note goes to the
    slot its timestep's counter points at unless the counter has reached 15 (dropped); pitch clamped to [0,127], duration to
    [1,96] and stored minus one; EOS at the counter; a timestep is active iff its counter moved.  Then the bars: an empty one
    gets cell [0,0]; the nodes are the active cells in (piece, bar, track, step) order."""
    notes, ptr = np.asarray(notes).astype(np.int64).reshape(-1, 3), np.asarray(track_ptr).astype(np.int64)
    B, length = (len(ptr) - 1) // 4, 32 * n_bars
    content = np.empty((B, 4, length, 16, 2), np.int64)
    content[...] = PAD
    content[:, :, :, 0] = SOS
    counter = np.ones((B, 4, length), np.int64)
    dropped = 0
    for i in range(B):
        for k in range(4):
            for t, pitch, dur in notes[ptr[4 * i + k]:ptr[4 * i + k + 1]]:
                if counter[i, k, t] >= 15:
                    dropped += 1
                    continue
                content[i, k, t, counter[i, k, t]] = (max(min(pitch, 127), 0), max(min(dur, 96), 1) - 1)
                counter[i, k, t] += 1
    ii, kk, tt = np.indices(counter.shape)
    content[ii, kk, tt, counter] = EOS
    # (track, time) -> (bar, track, step), data.py:226-233
    s = (counter > 1).reshape(B, 4, n_bars, 32).transpose(0, 2, 1, 3).copy()
    content = content.reshape(B, 4, n_bars, 32, 16, 2).transpose(0, 2, 1, 3, 4, 5)
    empty = ~s.any(axis=(2, 3))
    s[empty, 0, 0] = True
    return s.reshape(B * n_bars, 4, 32).astype(np.float32), content[s].astype(np.int32), dropped


def check_ref(notes, track_ptr, n_bars):
    """(rows out of time range, rows out of order, bad track_ptr entries) as `pm_tokens_from_notes` counts them: every track's
    range clamped into [0, M]; inside it a row whose time is outside [0, 32 n_bars), a row whose time is above the next
    row's; entry 0 of track_ptr unless it is 0, a later entry outside [0, M] or below the entry before it."""
    notes, ptr = np.asarray(notes).astype(np.int64).reshape(-1, 3), np.asarray(track_ptr).astype(np.int64)
    M = len(notes)
    out_of_range = out_of_order = 0
    for tr in range(len(ptr) - 1):
        lo = min(max(ptr[tr], 0), M)
        hi = min(max(ptr[tr + 1], lo), M)
        t = notes[lo:hi, 0]
        out_of_range += int(((t < 0) | (t >= 32 * n_bars)).sum())
        out_of_order += int((t[:-1] > t[1:]).sum())
    bad = int(ptr[0] != 0) + int(((ptr[1:] < 0) | (ptr[1:] > M) | (ptr[1:] < ptr[:-1])).sum())
    return out_of_range, out_of_order, bad


def end_clamped(tokens, s_tensor, n_bars):
    """the node tokens [N,16,2] a round trip through `notes_ref` gives back: every note's duration token d replaced by
    min(d + 1, 32 n_bars - t) - 1, t the time of its cell (the reference cuts a note at the end of the piece when it reads
    the pianoroll, utils.py:116-118)"""
    out = np.array(tokens, np.int32)
    s = np.asarray(s_tensor).reshape(-1, n_bars, 4, 32) != 0
    _, b, _, step = np.nonzero(s)
    left = (32 * n_bars - (32 * b + step))[:, None]                              # per node, node order
    note = out[..., 0] < 128
    out[..., 1] = np.where(note, np.minimum(out[..., 1] + 1, left) - 1, out[..., 1])
    return out


def as_batch(pieces):
    """lists (per piece, four lists of (time, pitch, duration)) -> (notes int32 [M,3], track_ptr int32 [4B+1]), each track
    stable-sorted by time: what `NoteBatch.from_lists` uploads"""
    rows, ptr = [], [0]
    for piece in pieces:
        for track in piece:
            rows.extend(sorted(track, key=lambda r: r[0]))
            ptr.append(len(rows))
    return np.asarray(rows, np.int32).reshape(-1, 3), np.asarray(ptr, np.int32)
