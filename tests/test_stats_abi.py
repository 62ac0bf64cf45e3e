"""Checks of the note statistics that need no GPU: pm_note_stats and pm_notes_select are declared in include/polyphemus_hip.h
("Note statistics", behind "Infill"), exported by the library and bound in the ctypes table with the header's argument lists,
the ABI version is unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can
stand in for device addresses), the Python surface rejects bad arguments without a device, and the numpy restatement the GPU
tests compare with (tests/stats_util.py) is tied down by a piece computed by hand and by the reference's recorded notes."""
import os
import re
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from notes_util import CASES, GOLDEN, load_notes
from stats_util import FIELDS, derived_ref, select_ref, stats_ref
from test_abi import HEADER, header_prototypes

SIGS = {"pm_note_stats": "ppiilpppps", "pm_notes_select": "ppilpiplpppps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
NOTES, PTR, TRACK, PC, ONSETS, SOUNDING, INDEX, OUT, OUT_PTR, TOTALS, SCRATCH, STATUS = (0x10000000 + k * 0x100000 for k in range(12))
B, NB, M, K, CAP = 3, 2, 50, 2, 40
T = 4 * B
N_SCRATCH = B + 16 * K
GOOD_S = dict(notes=NOTES, track_ptr=PTR, B=B, n_bars=NB, M=M, track=TRACK, pitch_class=PC, onsets=ONSETS, sounding=SOUNDING)
GOOD_L = dict(notes=NOTES, track_ptr=PTR, B=B, M=M, index=INDEX, K=K, out_notes=OUT, capacity=CAP, out_track_ptr=OUT_PTR,
              out_totals=TOTALS, scratch=SCRATCH, status=STATUS)
# words of every buffer, inputs first
WORDS_S = dict(notes=3 * M, track_ptr=T + 1, track=12 * T, pitch_class=12 * T, onsets=NB * T, sounding=NB * T)
WORDS_L = dict(notes=3 * M, track_ptr=T + 1, index=K, out_notes=3 * CAP, out_track_ptr=4 * K + 1, out_totals=2, scratch=N_SCRATCH,
               status=2)


def _stats(**kw):
    return _lib.lib().pm_note_stats(*{**GOOD_S, **kw}.values(), None)


def _select(**kw):
    return _lib.lib().pm_notes_select(*{**GOOD_L, **kw}.values(), None)


def test_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig and len(getattr(L, name).argtypes) == len(sig) and name in _lib.EXPORTED
    src = open(HEADER).read()
    assert (src.index("------ Infill") < src.index("------ Note statistics") < src.index("int pm_note_stats")
            < src.index("int pm_notes_select") < src.index("------ message aggregation"))
    section = src[src.index("------ Note statistics"):src.index("------ message aggregation")]
    for i, name in enumerate(FIELDS):
        assert re.search(rf"#define PM_NOTE_STAT_{name.upper()} {i}\n", section), name
    assert re.search(r"#define PM_SELECT_SCRATCH\(B, K\) \(\(int64_t\)\(B\) \+ 16 \* \(int64_t\)\(K\)\)", section)
    from polyphemus_amd import ops
    assert ops.NOTE_STAT_FIELDS == FIELDS
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


def _overlaps(good, words, inputs):
    """every written buffer put on the first and on the last word of every other buffer (inputs and outputs alike)"""
    bad = []
    for name in words:
        if name in inputs:
            continue
        for other, n in words.items():
            if other != name:
                bad += [{name: good[other]}, {name: good[other] + 4 * (n - 1)}]
        # ... and an input put on the last word of this output
        bad += [{i: good[name] + 4 * (words[name] - 1)} for i in inputs]
    return bad


BAD_S = ([dict(track_ptr=None), dict(track=None), dict(pitch_class=None), dict(onsets=None), dict(sounding=None), dict(notes=None),
          dict(B=0), dict(B=-3), dict(n_bars=0), dict(n_bars=-1), dict(n_bars=65), dict(n_bars=1 << 20), dict(M=-1), dict(M=-(1 << 40)),
          dict(M=(1 << 31) // 3 + 1), dict(M=1 << 62), dict(B=1 << 26, n_bars=8), dict(B=1 << 29, n_bars=1), dict(B=(1 << 31) // 48 + 1, n_bars=1),
          dict(notes=NOTES + 2), dict(track_ptr=PTR + 1), dict(track=TRACK + 2), dict(pitch_class=PC + 3), dict(onsets=ONSETS + 1),
          dict(sounding=SOUNDING + 2)] + _overlaps(GOOD_S, WORDS_S, ("notes", "track_ptr")))
BAD_L = ([dict(notes=None), dict(track_ptr=None), dict(index=None), dict(out_notes=None), dict(out_track_ptr=None), dict(out_totals=None),
          dict(scratch=None), dict(status=None), dict(B=0), dict(B=-1), dict(K=0), dict(K=-2), dict(M=-1), dict(capacity=-1),
          dict(M=(1 << 31) // 3 + 1), dict(M=1 << 62), dict(capacity=(1 << 31) // 3 + 1), dict(capacity=1 << 62), dict(B=1 << 29),
          dict(K=1 << 27), dict(B=(1 << 31) - 1),
          dict(notes=NOTES + 2), dict(track_ptr=PTR + 1), dict(index=INDEX + 2), dict(out_notes=OUT + 1), dict(out_track_ptr=OUT_PTR + 2),
          dict(out_totals=TOTALS + 3), dict(scratch=SCRATCH + 2), dict(status=STATUS + 1)]
         + _overlaps(GOOD_L, WORDS_L, ("notes", "track_ptr", "index")))
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_S, ids=_ids)
def test_note_stats_rejects_on_the_host(bad):
    assert _stats(**bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_L, ids=_ids)
def test_notes_select_rejects_on_the_host(bad):
    assert _select(**bad) == PM_E_INVALID


def test_no_rows_still_check_everything_else():
    """M == 0: notes may be NULL (capacity == 0: out_notes too); the other arguments are checked as ever"""
    for bad in (dict(track=None), dict(n_bars=65), dict(onsets=SOUNDING), dict(sounding=SOUNDING + 2)):
        assert _stats(M=0, notes=None, **bad) == PM_E_INVALID
    for bad in (dict(status=None), dict(K=0), dict(status=SCRATCH), dict(out_totals=TOTALS + 2)):
        assert _select(M=0, notes=None, **bad) == PM_E_INVALID
        assert _select(M=0, notes=None, capacity=0, out_notes=None, **bad) == PM_E_INVALID


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import NoteBatch, NoteStats, pick_takes
    nb = NoteBatch.from_lists([[[(0, 60, 4)], [], [(5, 41, 2)], []]] * 2, 2, device="cpu")
    notes, ptr = nb.notes, nb.track_ptr
    for a, b, name in ((notes.numpy(), ptr, "notes"), (notes.long(), ptr, "notes"), (notes.reshape(-1), ptr, "notes"), (notes[:, :2], ptr, "notes"),
                       (notes, ptr.tolist(), "track_ptr"), (notes, ptr.long(), "track_ptr"), (notes, ptr[:8], "track_ptr"), (notes, ptr[:1], "track_ptr"),
                       (notes, ptr.view(1, -1), "track_ptr")):
        with pytest.raises(ValueError, match=name):
            ops.note_stats(a, b, 2)
        with pytest.raises(ValueError, match=name):
            ops.notes_select(a, b, [0])
    for bad in (0, -1, 65, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="n_bars"):
            ops.note_stats(notes, ptr, bad)
    for bad in ([], (), [0.5], [True], "0", None, 1, torch.zeros(0, dtype=torch.int64), torch.zeros(2, dtype=torch.float32),
                torch.zeros(1, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int16), [1 << 31], np.zeros(2, np.int64)):
        with pytest.raises(ValueError, match="index"):
            ops.notes_select(notes, ptr, bad)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.note_stats(notes, ptr, 2)
    for index in ([0], [1, 0], torch.tensor([0]), torch.tensor([1], dtype=torch.int32)):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            ops.notes_select(notes, ptr, index)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        nb.stats()
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        nb.select([0])
    # pick_takes: before the model is touched
    z, key = torch.zeros(2, 8), lambda st: st.track[:, 1, 9].float()
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="takes"):
            pick_takes(None, z, bad, key)
    with pytest.raises(ValueError, match="return_tokens"):
        pick_takes(None, z, 2, key, return_tokens=False)
    with pytest.raises(ValueError, match="key"):
        pick_takes(None, z, 2, None)
    for bad in (None, z[0], torch.zeros(0, 8), z.numpy()):
        with pytest.raises(ValueError, match="z must be"):
            pick_takes(None, bad, 2, key)
    # generate_notes' own checks still come before the model
    for kw, name in ((dict(temperature=-1.0), "temperature"), (dict(top_k=0), "top_k"), (dict(chord_rules=3), "chord_rules")):
        with pytest.raises(ValueError, match=name):
            pick_takes(None, z, 2, key, **kw)
    st = NoteStats(torch.zeros(1, 4, 12, dtype=torch.int32), torch.zeros(1, 4, 12, dtype=torch.int32), torch.zeros(1, 4, 2, dtype=torch.int32),
                   torch.zeros(1, 4, 2, dtype=torch.int32), 2, resolution=5)
    with pytest.raises(ValueError, match="resolution"):
        st.empty_beat_rate()


HAND = [[(0, 60, 8), (0, 64, 8), (0, 67, 8), (31, 60, 500)],          # a C-major triad, a C that is cut at the end of the piece
        [(4, 60, 2), (4, 61, 2), (4, 62, 2), (5, 63, 1)],              # a chromatic cluster
        [],
        [(64, 50, 4), (-1, 50, 4)]]                                    # outside the piece


def test_restatement_on_a_piece_computed_by_hand():
    rows = [r for track in HAND for r in track]
    ptr = np.cumsum([0] + [len(t) for t in HAND]).astype(np.int32)
    track, pc, onsets, sounding = stats_ref(np.asarray(rows, np.int32), ptr, 2)
    assert all(a.dtype == np.int32 for a in (track, pc, onsets, sounding))
    #                          notes onsets min max pitches classes note_steps sounding poly max_poly max_chord out_of_range
    assert track.tolist() == [[4, 2, 60, 67, 3, 3, 24 + 33, 8 + 33, 8, 3, 3, 0],
                              [4, 2, 60, 63, 4, 4, 7, 2, 2, 4, 3, 0],
                              [0, 0, 128, -1, 0, 0, 0, 0, 0, 0, 0, 0],
                              [0, 0, 128, -1, 0, 0, 0, 0, 0, 0, 0, 2]]
    assert pc.tolist() == [[2, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0], [0] * 12, [0] * 12]
    assert onsets.tolist() == [[-2147483647, 0], [48, 0], [0, 0], [0, 0]]                   # bits 0 and 31; bits 4 and 5
    assert sounding.tolist() == [[-2147483648 + 255, -1], [48, 0], [0, 0], [0, 0]]          # steps 0..7 and 31, all of bar 1
    d = derived_ref(track, pc, onsets, sounding, 2, resolution=8)
    assert d["polyphony"].tolist() == [[57 / 41, 3.5, 0.0, 0.0]]
    assert d["polyphony_rate"].tolist() == [[0.125, 0.03125, 0.0, 0.0]]
    assert d["pitch_class_entropy"].tolist() == [[1.5, 2.0, 0.0, 0.0]]
    assert d["scale_consistency"].tolist() == [[1.0, 0.75, 0.0, 0.0]]                       # (D flat major holds 0, 1 and 3)
    assert d["groove_consistency"].tolist() == [[0.9375, 0.9375, 1.0, 1.0]]
    assert d["empty_beat_rate"].tolist() == [0.25]                                          # beats 1 and 2 of bar 0
    assert derived_ref(track, pc, onsets, sounding, 2, resolution=32)["empty_beat_rate"].tolist() == [0.0]
    # row order does not matter, nor do rows behind the last track
    back = np.asarray([r for t in HAND for r in t[::-1]] + [(0, 1, 1)] * 3, np.int32)
    assert all(np.array_equal(a, b) for a, b in zip(stats_ref(back, ptr, 2), (track, pc, onsets, sounding)))
    # one bar: the triad alone; the C at step 31 is cut to one step
    one = stats_ref(np.asarray(rows, np.int32), ptr, 1)
    assert one[0][0].tolist() == [4, 2, 60, 67, 3, 3, 25, 9, 8, 3, 3, 0] and one[0][3, 11] == 2
    assert derived_ref(*one, 1)["groove_consistency"].tolist() == [[1.0] * 4]
    # the subset: pieces (1, out of range, 0, 1 again) of two copies
    notes2, ptr2 = np.asarray(rows + rows, np.int32), np.concatenate([ptr, ptr[1:] + ptr[-1]])
    got, got_ptr, totals, status = select_ref(notes2, ptr2, [1, 2, 0, 1])
    assert np.array_equal(got, notes2) and got_ptr.tolist() == ptr.tolist() + [10] * 4 + (ptr[1:] + 10).tolist() + [20] * 4
    assert totals == [20, 2 * (2 + 2 + 0 + 2)] and status == [1, 1]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_on_the_recorded_reference_notes(name):
    B, n_bars = CASES[name]
    notes, ptr = load_notes(name)
    s = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)["in/s_tensor"].reshape(B, n_bars, 4, 32) != 0
    track, pc, onsets, sounding = stats_ref(notes, ptr, n_bars)
    assert track[:, 0].tolist() == np.diff(ptr).tolist() and not track[:, 11].any()
    assert np.array_equal(pc.sum(1), track[:, 0])
    for tr in range(4 * B):
        i, k = divmod(tr, 4)
        times = set(notes[ptr[tr]:ptr[tr + 1], 0].tolist())
        assert track[tr, 1] == len(times)
        bits = (onsets[tr].astype(np.int64)[:, None] >> np.arange(32)) & 1                   # [n_bars,32]
        assert bits.sum() == len(times) and not (bits.astype(bool) & ~s[i, :, k]).any()      # a subset of the structure's cells
        sound = (sounding[tr].astype(np.int64)[:, None] >> np.arange(32)) & 1
        assert not (bits & ~sound).any() and sound.sum() == track[tr, 7]
        # the recorded durations are cut at the end of the piece already: note_steps is their sum where none is above 96
        if (notes[ptr[tr]:ptr[tr + 1], 2] <= 96).all():
            assert track[tr, 6] == notes[ptr[tr]:ptr[tr + 1], 2].sum()
    assert track[:, 10].max() <= 15 and track[:, 9].max() >= 2
