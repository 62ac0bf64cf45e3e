"""The numpy restatement of note splicing (tests/splice_util.py) tied to cases computed by hand: a 3-bar song cut into windows
of 2 bars, the reference's silence filter on hand-made activity grids (the cross-track case among them), the transposition,
and the windows joined again.  No GPU."""
import itertools

import numpy as np

from splice_util import filter_ref, join_np, shift_ref, splice_ref, transposed, window_acts, windows_np

#        Drums                                  Bass                         Guitar  Strings (not sorted by time)
SONG = [[(0, 36, 4), (40, 38, 4), (70, 36, 4)], [(31, 40, 100), (32, 41, 2)], [], [(95, 60, 1), (64, 62, 1)]]
WINDOWS = [[[(0, 36, 4), (40, 38, 4)], [(31, 40, 100), (32, 41, 2)], [], []],                   # bars 0-1: a note is never cut
           [[(8, 38, 4), (38, 36, 4)], [(0, 41, 2)], [], [(63, 60, 1), (32, 62, 1)]]]           # bars 1-2: the order is kept


def flat(pieces):
    rows = [r for piece in pieces for track in piece for r in track]
    ptr = np.cumsum([0] + [len(track) for piece in pieces for track in piece]).astype(np.int32)
    return np.asarray(rows, np.int32).reshape(-1, 3), ptr


def test_restatement_on_a_song_cut_by_hand():
    notes, ptr = flat([SONG])
    segments, seg_ptr = [(0, 0, 0, 2), (0, 1, 0, 2)], [0, 1, 2]
    rows, out_ptr, totals, keep, status = splice_ref(notes, ptr, 3, segments, seg_ptr, 2, silence_rule=True)
    want, want_ptr = flat(WINDOWS)
    assert rows.dtype == np.int32 and np.array_equal(rows, want) and out_ptr.tolist() == want_ptr.tolist() == [0, 2, 4, 4, 4, 6, 7, 7, 9]
    assert totals == [9, 4 + 5] and status == [0, 0]
    assert keep == [0, 0]                                           # the guitar is silent in both bars of both windows
    assert splice_ref(notes, ptr, 3, segments, seg_ptr, 2)[3] == [1, 1]
    # the host route gives the same windows
    got, song, start = windows_np([SONG], 2, 1, total_bars=3)
    assert got == WINDOWS and song == [0, 0] and start == [0, 1]
    assert windows_np([SONG], 2, 2, total_bars=3)[0] == WINDOWS[:1] and windows_np([SONG], 2, 1, song_bars=[2])[0] == WINDOWS[:1]
    assert windows_np([SONG], 2, 1, song_bars=[1]) == ([], [], [])
    # shifts +3 and -100: the drums stay, the others are clamped
    rows, _, _, _, _ = splice_ref(notes, ptr, 3, segments, seg_ptr, 2, shift=[3, -100])
    assert rows[:, 1].tolist() == [36, 38, 43, 44, 38, 36, 0, 0, 0]
    assert transposed(WINDOWS[0], 3) == [WINDOWS[0][0], [(31, 43, 100), (32, 44, 2)], [], []]
    assert shift_ref([-3, 200, 125, 2], 6).tolist() == [6, 127, 127, 8] and shift_ref([-3, 200, 125, 2], -5).tolist() == [0, 122, 120, 0]
    assert shift_ref([-3, 200], 0).tolist() == [0, 127]
    # segments that are not followed copy nothing: bad piece, negative bar, overrun of source and output, overlap, no bars
    for bad in ((1, 0, 0, 2), (-1, 0, 0, 2), (0, -1, 0, 2), (0, 2, 0, 2), (0, 0, 1, 2), (0, 0, 0, 0), (0, 0, -1, 1)):
        rows, out_ptr, totals, _, status = splice_ref(notes, ptr, 3, [bad], [0, 1], 2)
        assert len(rows) == 0 and out_ptr.tolist() == [0] * 5 and totals == [0, 0] and status == [1, 0], bad
    rows, out_ptr, _, _, status = splice_ref(notes, ptr, 3, [(0, 0, 0, 1), (0, 2, 0, 1), (0, 1, 1, 1)], [0, 3], 2)
    assert status == [1, 0] and rows.tolist() == [[0, 36, 4], [40, 38, 4], [31, 40, 100], [32, 41, 2]]   # the second overlaps the first
    # seg_ptr is clamped and counted
    rows, out_ptr, _, _, status = splice_ref(notes, ptr, 3, segments, [-1, 5, 1], 2)
    assert status == [1, 3] and out_ptr.tolist() == [0, 2, 4, 4, 4, 4, 4, 4, 4]     # piece 0: both segments, the second overlaps; piece 1: none


def test_windows_joined_again_are_the_song():
    sorted_song = [sorted(t, key=lambda r: r[0]) for t in SONG]
    wins, _, _ = windows_np([sorted_song], 1, 1, total_bars=3)
    assert join_np(wins, [[0, 1, 2]], 1) == [sorted_song]
    two, _, _ = windows_np([sorted_song], 2, 1, total_bars=3)
    assert join_np(two, [[0, 1]], 2, hop=1) == [sorted_song]
    assert join_np(two, [[1, -1, 0]], 2) == [[[(8, 38, 4), (38, 36, 4), (128, 36, 4), (168, 38, 4)], [(0, 41, 2), (159, 40, 100), (160, 41, 2)],
                                              [], [(32, 62, 1), (63, 60, 1)]]]
    # the restatement of the kernel on the segments `join` builds
    notes, ptr = flat(two)
    rows, out_ptr, totals, _, status = splice_ref(notes, ptr, 2, [(0, 0, 0, 1), (1, 0, 1, 2)], [0, 2], 3)
    want, want_ptr = flat([sorted_song])
    assert np.array_equal(rows, want) and out_ptr.tolist() == want_ptr.tolist() and status == [0, 0] and totals == [7, 7]


def grid(*rows):
    return np.asarray(rows, bool)


def test_filter_on_grids_made_by_hand():
    assert filter_ref(grid([1, 1], [1, 1], [1, 1], [1, 1]))
    assert filter_ref(grid([1, 0], [1, 1], [1, 1], [0, 1]))                      # silent bars 1 then 0: the difference is -1
    assert filter_ref(grid([1, 0, 1], [0, 1, 1], [1, 1, 1], [1, 1, 0]))          # 1, 0, 2
    assert not filter_ref(grid([0, 0], [1, 1], [1, 1], [1, 1]))                  # two consecutive silent bars of a track
    assert not filter_ref(grid([1, 1, 1], [1, 1, 1], [1, 0, 0], [1, 1, 1]))
    assert not filter_ref(grid([1, 0], [1, 0], [1, 0], [1, 0]))                  # a bar silent in every track (differences 0)
    # the cross-track case: no track has two silent bars, no bar is silent in all, and still 0 -> 1 follow each other
    assert not filter_ref(grid([0, 1], [1, 0], [1, 1], [1, 1]))
    assert not filter_ref(grid([0, 1, 1], [1, 1, 1], [1, 0, 1], [1, 1, 1]))      # ... across a track without a silent bar
    assert filter_ref(grid([1, 0, 1, 0], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]))                 # 1, 3: kept
    assert filter_ref(grid([1, 0, 1, 0], [0, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]))                 # 1, 3, 0: kept
    assert not filter_ref(grid([1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1], [1, 1, 1, 1]))             # 1, 2 across tracks
    # one bar: only all four silent is rejected
    assert not filter_ref(grid([0], [0], [0], [0]))
    assert filter_ref(grid([0], [0], [1], [0])) and filter_ref(grid([1], [1], [1], [1]))
    assert window_acts([[(0, 1, 1)], [], [(33, 1, 1), (63, 1, 1)], []], 2).tolist() == [[True, False], [False, False], [False, True], [False, False]]


def keeps_masks(masks, W):
    """the rule as the kernel states it, on the four bit masks of a piece (bit b: the track has a row in bar b)"""
    full = (1 << W) - 1
    every = masks[0] | masks[1] | masks[2] | masks[3]
    if W == 1:
        return bool(every & 1)
    if ~every & full:
        return False
    prev_last = -2
    for m in masks:
        silent = ~m & full
        if not silent:
            continue
        if silent & (silent >> 1):
            return False
        if (silent & -silent).bit_length() - 1 == prev_last + 1:
            return False
        prev_last = silent.bit_length() - 1
    return True


def test_the_mask_form_of_the_filter_is_the_literal_expression_on_every_small_grid():
    for W in (1, 2, 3, 4):
        for masks in itertools.product(range(1 << W), repeat=4):
            acts = [[(m >> b) & 1 for b in range(W)] for m in masks]
            assert keeps_masks(masks, W) == filter_ref(np.asarray(acts, bool)), (W, masks)
