#!/usr/bin/env python3
"""Record the notes the reference reads out of a generated pianoroll: tests/golden/<case>_notes.npz.

Runs on the CPU where the reference checkout is available (REF below, as oracle/make_golden.py); no test imports it.  For
the cases lmd2_tiny (B = 8, two bars) and nb3_tiny (B = 6, three bars) it takes `eval/c_logits` and `in/s_tensor` from
tests/golden/<case>.npz, runs the reference's own `mtp_from_logits` and `muspy_from_mtp` (utils.py:59-141) on every piece
and writes
    notes      int32 [M,3]     (time, pitch, duration), piece after piece, track after track, in the reference's order
    track_ptr  int32 [4B+1]    the rows of (piece i, track k) are notes[track_ptr[4i+k]:track_ptr[4i+k+1]]
The stub `muspy` of oracle/pyg_shim is empty: the four record classes `muspy_from_mtp` builds are given to it here.  Only
recorded numbers are written, nothing of the reference's code.  The assertions keep a regenerated fixture from going
hollow: enough notes, a clamped duration, and for nb3_tiny a skipped SOS pitch and a duration token 96.

Usage: python tools/make_notes_golden.py        (from anywhere; PM_GOLDEN_OUT overrides the output folder)"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, "oracle", "pyg_shim"))

import muspy  # noqa: E402  (the empty stub)


class _Record:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Note(_Record):
    def __init__(self, time, pitch, duration, velocity):
        super().__init__(time=time, pitch=pitch, duration=duration, velocity=velocity)


class Track(_Record):
    pass


class Metadata(_Record):
    pass


class Music(_Record):
    pass


muspy.Note, muspy.Track, muspy.Metadata, muspy.Music = Note, Track, Metadata, Music

_cwd = os.getcwd()
os.chdir(REF)                    # generation_config.py opens its yaml relative to the working directory
import utils as ref_utils        # noqa: E402
os.chdir(_cwd)

GOLDEN = os.path.join(REPO, "tests", "golden")
OUT = os.environ.get("PM_GOLDEN_OUT", GOLDEN)
CASES = {"lmd2_tiny": (8, 2), "nb3_tiny": (6, 3)}
TRACKS = ["Drums", "Bass", "Guitar", "Strings"]


def record(case, B, n_bars):
    z = np.load(os.path.join(GOLDEN, f"{case}.npz"), allow_pickle=False)
    c_logits = torch.from_numpy(z["eval/c_logits"]).float()
    s_tensor = torch.from_numpy(z["in/s_tensor"]).reshape(B, n_bars, 4, 32)
    assert int(s_tensor.sum()) == c_logits.shape[0]
    mtp = ref_utils.mtp_from_logits(c_logits, s_tensor)
    rows, track_ptr = [], [0]
    for i in range(B):
        music = ref_utils.muspy_from_mtp(mtp[i])
        assert music.resolution == 8 and [t.name for t in music.tracks] == TRACKS
        assert [t.is_drum for t in music.tracks] == [True, False, False, False]
        for track in music.tracks:
            assert all(n.velocity == 64 for n in track.notes)
            rows += [(int(n.time), int(n.pitch), int(n.duration)) for n in track.notes]
            track_ptr.append(len(rows))
    notes = np.asarray(rows, np.int32).reshape(-1, 3)
    # what the arg-max tokens hold, for the assertions below (the recording itself is the reference's)
    pitch, dur = c_logits[..., :131].argmax(-1).numpy(), c_logits[..., 131:].argmax(-1).numpy()
    ended = np.cumsum(np.isin(pitch, (129, 130)) | np.isin(dur, (97, 98)), axis=1) > 0
    sos_skips, dur_sos = int(((pitch == 128) & ~ended).sum()), int((dur == 96).sum())
    clamped = _count_clamped(pitch, dur, ended, s_tensor, n_bars)
    M = notes.shape[0]
    print(f"{case}: M = {M}, {clamped} clamped durations, {sos_skips} skipped SOS pitches, {dur_sos} duration tokens 96")
    assert M >= 1000, M
    assert ((notes[:, 0] + notes[:, 2]) <= 32 * n_bars).all() and (notes[:, 2] >= 1).all()
    assert clamped >= 1, clamped
    if case == "nb3_tiny":
        assert sos_skips >= 1 and dur_sos >= 1, (sos_skips, dur_sos)
    np.savez_compressed(os.path.join(OUT, f"{case}_notes.npz"), notes=notes, track_ptr=np.asarray(track_ptr, np.int32))


def _count_clamped(pitch, dur, ended, s_tensor, n_bars):
    """notes whose duration token + 1 exceeds what is left of the piece at their time"""
    cells = np.argwhere(s_tensor.reshape(-1, 4, 32).numpy() != 0)                # node order = cell order: (bar, track, step)
    time = 32 * (cells[:, 0] % n_bars) + cells[:, 2]
    live = ~ended & (pitch != 128)
    return int((live & (dur + 1 > (32 * n_bars - time)[:, None])).sum())


if __name__ == "__main__":
    torch.set_num_threads(1)
    for name, (B, nb) in CASES.items():
        record(name, B, nb)
