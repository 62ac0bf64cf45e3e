"""The numpy restatement the note-event GPU tests lean on (`notes_ref`, tests/notes_util.py) against notes recorded from the
reference itself (tools/make_notes_golden.py: its `mtp_from_logits` + `muspy_from_mtp` on the golden cases), row for row.
No GPU."""
import numpy as np
import pytest

from notes_util import CASES, as_lists, load_case_tokens, load_notes, looped_ref, notes_ref


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_reference_recorded_notes(name):
    B, n_bars = CASES[name]
    tokens, s, _ = load_case_tokens(name)
    want, want_ptr = load_notes(name)
    assert want.dtype == np.int32 and want.shape[1:] == (3,) and want_ptr.dtype == np.int32 and want_ptr.shape == (4 * B + 1,)
    assert want.shape[0] >= 1000 and want_ptr[0] == 0 and want_ptr[-1] == want.shape[0] and (np.diff(want_ptr) >= 0).all()
    got, got_ptr = notes_ref(tokens, s)
    assert got.dtype == np.int32 and np.array_equal(got_ptr, want_ptr)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]


def test_fixtures_keep_the_branches_they_were_recorded_for():
    """clamped durations in both cases; in nb3_tiny skipped SOS pitches and duration tokens 96 inside live chords"""
    for name, (B, n_bars) in CASES.items():
        tokens, s, _ = load_case_tokens(name)
        notes, _ = load_notes(name)
        assert (notes[:, 0] + notes[:, 2] <= 32 * n_bars).all() and (notes[:, 2] >= 1).all()
        assert (notes[:, 0] + notes[:, 2] == 32 * n_bars).sum() > 0
    tokens, s, _ = load_case_tokens("nb3_tiny")
    ended = np.cumsum(np.isin(tokens[..., 0], (129, 130)) | np.isin(tokens[..., 1], (97, 98)), axis=1) > 0
    assert ((tokens[..., 0] == 128) & ~ended).sum() >= 1 and ((tokens[..., 1] == 96) & ~ended & (tokens[..., 0] < 128)).sum() >= 1


def test_restatement_on_hand_written_cells():
    s = np.zeros((1, 2, 4, 32), np.uint8)
    s[0, 0, 0, 3] = s[0, 0, 2, 0] = s[0, 1, 0, 31] = s[0, 1, 3, 5] = 1       # nodes 0 (drums t=3), 1 (guitar t=0), 2 (drums t=63), 3 (strings t=37)
    tok = np.full((4, 15, 2), (130, 98), np.int64)
    tok[0, :4] = [(36, 0), (128, 5), (40, 96), (129, 97)]                     # SOS skipped, duration 96 -> 97, clamped to 61
    tok[1, :3] = [(60, 98), (61, 1), (129, 97)]                               # a PAD duration ends the chord at once
    tok[2, :2] = [(38, 95), (-1, 99)]                                         # last step: clamped to 1; out of range -> (0, 0), then PAD
    tok[3, :] = [(50 + j, j) for j in range(15)]                              # 15 notes, no terminator
    notes, ptr = notes_ref(tok, s)
    assert ptr.tolist() == [0, 4, 4, 4, 19]
    assert notes[:4].tolist() == [[3, 36, 1], [3, 40, 61], [63, 38, 1], [63, 0, 1]]
    assert notes[4:].tolist() == [[37, 50 + j, j + 1] for j in range(15)]
    assert notes_ref(tok[:3], s)[1].tolist() == [0, 4, 4, 4, 4]              # node 3 is beyond N: silent
    pieces = as_lists(notes, ptr)
    assert len(pieces) == 1 and [len(t) for t in pieces[0]] == [4, 0, 0, 15] and pieces[0][0][1] == (3, 40, 61)
    loop = looped_ref(pieces, 3, 2)
    assert [len(t) for t in loop[0]] == [12, 0, 0, 45] and loop[0][0][4] == (67, 36, 1) and loop[0][0][8] == (131, 36, 1)
    assert looped_ref(pieces, 1, 2) == pieces
