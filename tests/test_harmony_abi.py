"""Checks of the harmony entries that need no GPU: pm_node_cells, pm_sample_chords_at and pm_note_chroma are declared in
include/polyphemus_hip.h ("Harmony", behind "Scores"), exported by the library and bound in the ctypes table with the
header's argument lists, the ABI version is unchanged, every argument check answers PM_E_INVALID on the host before any
launch (so host integers can stand in for device addresses), `Harmony.from_chords` gives hand-written sets, the Python
surface rejects bad arguments without a device, and the numpy restatements the GPU tests compare with
(tests/harmony_util.py) give hand-computed values."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from harmony_util import A_MINOR, C_MAJOR, C_MAJOR_SCALE, FREE, TRIADS, chroma_ref, sets_ref
from test_abi import HEADER, header_prototypes

SIGS = {"pm_node_cells": "pilppps", "pm_sample_chords_at": "pplpiipupps", "pm_note_chroma": "ppiliips"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
S, BAR_NODES, NODE_PTR, NODE_CELL, LOGITS, CHART, TOKENS, COUNT, NOTES, TRACK_PTR, CHROMA = (0x10000000 + k * 0x100000 for k in range(11))
RULES = _lib.PmChordRules()
RULES.temperature[0] = RULES.temperature[1] = 1.0
RULES.top_k, RULES.top_p = 0, 1.0
for _k in range(4):
    RULES.min_notes[_k], RULES.max_notes[_k] = 1, 14
    for _w in range(4):
        RULES.pitch_mask[_k][_w] = 0xFFFFFFFF
GOOD_C = dict(s_tensor=S, G=3, N=40, bar_nodes=BAR_NODES, node_ptr=NODE_PTR, node_cell=NODE_CELL)
GOOD_A = dict(c_logits=LOGITS, node_cell=NODE_CELL, N=40, chart=CHART, G=3, track_bits=14, rules=ctypes.addressof(RULES), seed=1,
              tokens=TOKENS, note_count=COUNT)
GOOD_H = dict(notes=NOTES, track_ptr=TRACK_PTR, B=2, M=10, n_bars=2, seg_steps=8, chroma=CHROMA)


def _cells(**kw):
    return _lib.lib().pm_node_cells(*{**GOOD_C, **kw}.values(), None)


def _at(**kw):
    return _lib.lib().pm_sample_chords_at(*{**GOOD_A, **kw}.values(), None)


def _chroma(**kw):
    return _lib.lib().pm_note_chroma(*{**GOOD_H, **kw}.values(), None)


def test_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig and len(getattr(L, name).argtypes) == len(sig) and name in _lib.EXPORTED
    src = open(HEADER).read()
    assert (src.index("------ Scores") < src.index("int pm_score_structure") < src.index("------ Harmony")
            < src.index("int pm_node_cells") < src.index("int pm_sample_chords_at") < src.index("int pm_note_chroma")
            < src.index("------ message aggregation"))
    section = src[src.index("------ Harmony"):src.index("------ message aggregation")]
    assert "generate.py:21-37" in section and "utils.py:126-141" in section
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()
    # the existing entries keep their argument lists
    assert protos["pm_sample_chords"] == "pplpupps" and protos["pm_node_tracks"] == "pilppps" and protos["pm_note_stats"] == "ppiilpppps"


_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())
BAD_C = ([{k: None} for k in ("s_tensor", "bar_nodes", "node_ptr", "node_cell")]
         + [dict(G=0), dict(G=-1), dict(N=-1), dict(N=-(1 << 40)), dict(node_ptr=BAR_NODES), dict(node_cell=NODE_CELL + 2),
            dict(node_cell=NODE_CELL + 1), dict(G=1 << 24), dict(G=(1 << 31) - 1)])
BAD_A = ([{k: None} for k in ("c_logits", "node_cell", "chart", "rules", "tokens")]
         + [dict(N=0), dict(N=-1), dict(N=(1 << 32) // 15 + 1), dict(N=1 << 62), dict(G=0), dict(G=-3), dict(G=1 << 24),
            dict(track_bits=-1), dict(track_bits=16), dict(track_bits=1 << 20), dict(c_logits=LOGITS + 2), dict(node_cell=NODE_CELL + 1),
            dict(chart=CHART + 2), dict(tokens=TOKENS + 3), dict(note_count=COUNT + 2)])
BAD_H = ([{k: None} for k in ("notes", "track_ptr", "chroma")]
         + [dict(B=0), dict(B=-2), dict(n_bars=0), dict(n_bars=65), dict(n_bars=-1), dict(seg_steps=0), dict(seg_steps=3),
            dict(seg_steps=64), dict(seg_steps=-8), dict(seg_steps=12), dict(M=-1), dict(M=(1 << 31) // 3 + 1), dict(M=1 << 62),
            dict(B=1 << 26, n_bars=64, seg_steps=1), dict(notes=NOTES + 2), dict(track_ptr=TRACK_PTR + 1), dict(chroma=CHROMA + 3),
            dict(chroma=NOTES), dict(chroma=TRACK_PTR + 4), dict(notes=CHROMA + 16)])


@pytest.mark.parametrize("bad", BAD_C, ids=_ids)
def test_node_cells_rejects_on_the_host(bad):
    assert _cells(**bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_A, ids=_ids)
def test_sample_chords_at_rejects_on_the_host(bad):
    assert _at(**bad) == PM_E_INVALID


@pytest.mark.parametrize("field,value", [("temperature", -1.0), ("temperature", float("nan")), ("temperature", float("inf")),
                                         ("top_k", -1), ("top_p", 0.0), ("top_p", 1.5), ("top_p", float("nan")),
                                         ("min_notes", -1), ("min_notes", 15), ("max_notes", 0), ("max_notes", 15)])
def test_sample_chords_at_rejects_the_rules_sample_chords_rejects(field, value):
    rules = _lib.PmChordRules.from_buffer_copy(RULES)
    if field in ("top_k", "top_p"):
        setattr(rules, field, value)
    else:
        getattr(rules, field)[1] = value
    assert _at(rules=ctypes.addressof(rules)) == PM_E_INVALID
    node_track = NODE_CELL
    assert _lib.lib().pm_sample_chords(LOGITS, node_track, 40, ctypes.addressof(rules), 1, TOKENS, COUNT, None) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_H, ids=_ids)
def test_note_chroma_rejects_on_the_host(bad):
    assert _chroma(**bad) == PM_E_INVALID


def test_no_notes_still_check_everything_else():
    """M == 0: notes may be NULL; the other arguments are checked as ever"""
    for bad in (dict(chroma=None), dict(track_ptr=None), dict(B=0), dict(n_bars=65), dict(seg_steps=5), dict(chroma=CHROMA + 1)):
        assert _chroma(M=0, notes=None, **bad) == PM_E_INVALID


def test_from_chords_against_hand_written_sets():
    from polyphemus_amd.generate import Harmony
    h = Harmony.from_chords(["C", "Am", "F#m7", "Bb", "N", "G7"], 6)
    assert h.sets.shape == (6, 1) and h.n_bars == 6 and h.per_bar == 1 and h.track_bits == 0b1110 and h.empty == "free"
    # C E G; A C E; F# A C# E; Bb D F; every class; G B D F
    assert h.sets.flatten().tolist() == [C_MAJOR, A_MINOR, 0x252, 0x424, FREE, 0x8A4] and C_MAJOR == 0x091 and A_MINOR == 0x211
    assert Harmony.from_chords(["C"], 1, scale="major").sets.tolist() == [[C_MAJOR_SCALE]] and C_MAJOR_SCALE == 0xAB5
    assert Harmony.from_chords(["Am"], 1, scale="minor").sets.tolist() == [[C_MAJOR_SCALE]]       # A natural minor: the same notes
    assert Harmony.from_chords(["Am"], 1, scale="major").sets.tolist() == [[0xB56]]               # A B C# D E F# G#
    two = Harmony.from_chords(["C", "G", "Dm", "N"], 2, per_bar=2, tracks=("Guitar",), empty="rest")
    assert two.sets.tolist() == [[0x091, 0x884], [0x224, FREE]] and two.track_bits == 0b0100 and two.empty == "rest"
    every = ["", "m", "7", "maj7", "m7", "dim", "aug", "sus2", "sus4", "5"]
    want = [0x091, 0x089, 0x491, 0x891, 0x489, 0x049, 0x111, 0x085, 0x0A1, 0x081]
    assert Harmony.from_chords(["C" + q for q in every] + ["N"] * 6, 16).sets.flatten().tolist()[:10] == want
    assert Harmony.from_chords(["Db", "C#", "Cb", "B#"], 4).sets.flatten().tolist() == [0x122, 0x122, 0x848, 0x091]
    for n_bars, per_bar in ((2, 1), (1, 1), (3, 2)):                              # a wrong length
        with pytest.raises(ValueError, match="symbols must hold"):
            Harmony.from_chords(["C", "Am", "F"], n_bars, per_bar)
    for bad in ("H", "Cmin", "c", "C##", "", "Am9", "N7", 7, None):
        with pytest.raises(ValueError, match="chord symbol " + re.escape(repr(bad))):
            Harmony.from_chords(["C", bad], 2)
    with pytest.raises(ValueError, match="per_bar"):
        Harmony.from_chords(["C"] * 3, 1, per_bar=3)
    with pytest.raises(ValueError, match="scale"):
        Harmony.from_chords(["C"], 1, scale="dorian")
    with pytest.raises(ValueError, match="n_bars"):
        Harmony.from_chords([], 0)
    with pytest.raises(ValueError, match="symbols"):
        Harmony.from_chords("C", 1)


def test_harmony_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import Harmony
    ok = np.full((2, 4), C_MAJOR)
    for bad in (np.zeros(4, np.int64), np.zeros((1, 2, 2, 4), np.int64), np.zeros((2, 3), np.int64), np.zeros((2, 64), np.int64),
                np.zeros((0, 4), np.int64), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 0, 4, dtype=torch.int64), 5):
        for make in (ops.check_harmony_args, Harmony):
            with pytest.raises(ValueError, match="sets must be"):
                make(bad)
    for bad in (np.full((2, 4), 4096), np.full((2, 4), -1), torch.full((1, 2, 1), 4096), [[1 << 40]], [[0, 4096]]):
        for make in (ops.check_harmony_args, Harmony):
            with pytest.raises(ValueError, match=r"values in \[0, 4096\)"):
                make(bad)
    for bad in (np.zeros((2, 4)), torch.zeros(2, 4), np.zeros((2, 4), bool), [["C"]], None):
        for make in (ops.check_harmony_args, Harmony):
            with pytest.raises(ValueError, match="sets must"):
                make(bad)
    for bad in (("Piano",), ("Bass", 4), (-1,), "Bass", 1, None, (1.0,), (True,)):
        for make in (ops.check_harmony_args, Harmony):
            with pytest.raises(ValueError, match="tracks"):
                make(ok, tracks=bad)
    for bad in ("none", None, 0, "Free"):
        for make in (ops.check_harmony_args, Harmony):
            with pytest.raises(ValueError, match="empty"):
                make(ok, empty=bad)
    sets, bits = ops.check_harmony_args([[1, 2]], tracks=("Drums", 3))
    assert sets.tolist() == [[1, 2]] and bits == 0b1001 and ops.check_harmony_args(ok, tracks=())[1] == 0
    with pytest.raises(ValueError, match="n_bars = 3"):
        ops.check_harmony_args(ok, n_bars=3)
    with pytest.raises(ValueError, match="B = 3"):
        ops.check_harmony_args(np.zeros((2, 2, 1), np.int64), B=3, n_bars=2)
    ops.check_harmony_args(ok, B=7, n_bars=2)                                     # shared sets fit every B


def test_chart_expansion_and_the_cuts_are_plain_torch():
    """`Harmony.chart`, `repeated` and `windows` are torch ops on whatever device the sets are sent to: checked here on the CPU"""
    from polyphemus_amd.generate import Harmony
    sets = np.array([[C_MAJOR, 0], [FREE, A_MINOR]])
    free = Harmony(torch.from_numpy(sets)).chart(3, 2, "cpu")
    assert free.dtype == torch.int32 and free.shape == (6, 32) and free.is_contiguous()
    want = np.repeat(np.array([[C_MAJOR, FREE], [FREE, A_MINOR]]), 16, axis=1)
    assert np.array_equal(free.numpy(), np.tile(want, (3, 1)))
    rest = Harmony(torch.from_numpy(sets), empty="rest").chart(1, 2, "cpu")
    assert np.array_equal(rest.numpy(), np.repeat(np.array([[C_MAJOR, 0], [FREE, A_MINOR]]), 16, axis=1))
    per_piece = Harmony(np.arange(1, 13).reshape(3, 2, 2))
    assert np.array_equal(per_piece.chart(3, 2, "cpu").numpy(), np.repeat(np.arange(1, 13).reshape(6, 2), 16, axis=1))
    with pytest.raises(ValueError, match="B = 2"):
        per_piece.chart(2, 2, "cpu")
    with pytest.raises(ValueError, match="n_bars = 4"):
        per_piece.chart(3, 4, "cpu")
    assert per_piece.repeated(2).sets.tolist() == per_piece.sets.repeat_interleave(2, 0).tolist()
    shared = Harmony(sets)
    assert shared.repeated(5) is shared
    # five bars of a song in windows of two: three windows per song, the sixth bar free
    song = Harmony(np.arange(1, 11).reshape(2, 5, 1), tracks=("Bass",), empty="rest").windows(2, 2)
    assert song.sets.shape == (6, 2, 1) and song.track_bits == 0b0010 and song.empty == "rest"
    assert song.sets.flatten().tolist() == [1, 2, 3, 4, 5, FREE, 6, 7, 8, 9, 10, FREE]
    assert Harmony(np.array([[3], [0], [5]])).windows(2, 2).sets.flatten().tolist() == [3, FREE, 5, FREE] * 2


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import (Harmony, NoteBatch, generate_music, generate_notes, infill_notes, pick_takes, region_mask,
                                         vary_notes, vary_song)
    x, cells, chart = torch.zeros(5, 15, 230), torch.zeros(5, dtype=torch.int32), torch.zeros(2, 32, dtype=torch.int32)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.sample_chords_at(x, cells, chart)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.node_cells(torch.zeros(1, 2, 4, 32), 0)
    with pytest.raises(ValueError, match="s_tensor"):
        ops.node_cells(torch.zeros(4, 31), 0)
    nb = NoteBatch.from_lists([[[(0, 60, 4)], [], [(5, 41, 2)], []]] * 2, 2, device="cpu")
    for bad in (0, 3, 64, 8.0, None, True):
        with pytest.raises(ValueError, match="seg_steps"):
            ops.note_chroma(nb.notes, nb.track_ptr, 2, bad)
    for bad in (0, 65, 1.0):
        with pytest.raises(ValueError, match="n_bars"):
            ops.note_chroma(nb.notes, nb.track_ptr, bad)
    with pytest.raises(ValueError, match="notes must be int32"):
        ops.note_chroma(nb.notes.long(), nb.track_ptr, 2)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        nb.chroma()
    with pytest.raises(ValueError, match="snap"):
        nb.harmony(snap="seventh")
    with pytest.raises(ValueError, match="tracks"):
        nb.harmony(tracks=("Piano",))

    # generate: before the model or the device is touched
    vae = types.SimpleNamespace(cfg=dict(n_bars=2, d=8), training=True)
    z = torch.zeros(2, 8)
    three_bars, three_pieces = Harmony.from_chords(["C", "F", "G"], 3), Harmony(np.zeros((3, 2, 1), np.int64))
    for fn in (generate_music, generate_notes):
        with pytest.raises(ValueError, match="n_bars = 2"):
            fn(vae, z, harmony=three_bars)
        with pytest.raises(ValueError, match="B = 2"):
            fn(vae, z, harmony=three_pieces)
        with pytest.raises(ValueError, match="harmony must be a Harmony"):
            fn(vae, z, harmony=[[0x091]])
        with pytest.raises(ValueError, match="top_k"):                            # the chord rules' checks run with a harmony
            fn(vae, z, harmony=Harmony.from_chords(["C", "F"], 2), top_k=0)
    with pytest.raises(ValueError, match="B = 2"):
        pick_takes(vae, z, 3, lambda st: st.polyphony().sum(1), harmony=three_pieces)
    for fn, args in ((vary_notes, ()), (infill_notes, (region_mask(2, tracks=["Guitar"]),)), (vary_song, ())):
        with pytest.raises(ValueError, match="n_bars = 2"):
            fn(vae, nb, *args, harmony=three_bars)
        with pytest.raises(ValueError, match="B = 2"):
            fn(vae, nb, *args, harmony=three_pieces)
    song = NoteBatch(nb.notes, nb.track_ptr, nb.totals, 5)
    with pytest.raises(ValueError, match="n_bars = 5"):
        vary_song(vae, song, harmony=three_bars)
    assert vae.training


def test_restatements_on_a_piece_computed_by_hand():
    """one piece of two bars: Bass holds C2 over steps 0..3 and a G cut at the piece's end, Strings an E from step 30 on across
    the bar line, a row outside the piece and a pitch that is clamped to 127 (class 7)"""
    notes = np.array([(0, 36, 4), (62, 43, 10), (30, 64, 6), (64, 60, 4), (-1, 60, 4), (8, 300, 1)], np.int32)
    ptr = np.array([0, 0, 2, 2, 6], np.int32)
    c32 = chroma_ref(notes, ptr, 2, 32)
    assert c32.shape == (4, 2, 12) and c32.dtype == np.int32 and c32.sum() == 4 + 2 + 6 + 1
    assert c32[1, 0, 0] == 4 and c32[1, 1, 7] == 2 and c32[3, 0, 4] == 2 and c32[3, 1, 4] == 4 and c32[3, 0, 7] == 1
    c8 = chroma_ref(notes, ptr, 2, 8)
    assert c8.shape == (4, 8, 12) and np.array_equal(c8.reshape(4, 2, 4, 12).sum(2), c32)
    assert c8[3, 3, 4] == 2 and c8[3, 4, 4] == 4 and c8[3, 1, 7] == 1
    assert np.array_equal(chroma_ref(notes, ptr, 2, 1).reshape(4, 2, 32, 12).sum(2), c32)
    # a track_ptr that points outside [0, M] is clamped
    assert np.array_equal(chroma_ref(notes, np.array([-4, 0, 2, 2, 99], np.int32), 2, 32), c32)
    sets = sets_ref(c32.reshape(1, 4, 2, 12), (1, 3))
    assert sets.tolist() == [[0x091, 0x090]]
    assert sets_ref(c32.reshape(1, 4, 2, 12), (0, 2)).tolist() == [[0, 0]]
    # C + E + G: C major.  E + G alone: weight 4 + 2 inside C major and inside E minor, the major template comes first
    assert TRIADS[0] == C_MAJOR and TRIADS[12 + 9] == A_MINOR and len(set(TRIADS)) == 24
    assert sets_ref(c32.reshape(1, 4, 2, 12), (1, 3), snap="triad").tolist() == [[C_MAJOR, C_MAJOR]]
