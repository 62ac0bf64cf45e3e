"""Host mirror of the reference's generation entry points (generate.py:21-37, 90-98) over the device kernels of
csrc/generate.hip and csrc/graph.hip: the decoder pass, the thresholded structure, and the dense multitrack pianoroll,
without the reference's host synchronisations (`nonzero`, per-sample Python graph building, three full-tensor writes).
Converting the pianoroll to MIDI (muspy) is outside the hot path and stays with the caller; `generate_notes` returns the
pieces as ordered note events instead (`NoteBatch`, csrc/notes.hip), which is what that conversion reads out of the pianoroll.
The other direction has no entry point in the reference: `NoteBatch.from_lists` / `to_graph` (csrc/notes_in.hip) turn notes into the
batch the encoder consumes, `encode_notes` and `vary_notes` encode a piece and decode around it, `infill_notes` regenerates the
cells of a region (`region_mask`) and keeps the other notes (csrc/infill.hip).  `NoteBatch.stats` counts what the pieces hold on the
device (`NoteStats`, csrc/stats.hip), `NoteBatch.select` takes a subset of them, `pick_takes` keeps the best of several takes.
`NoteBatch.windows` cuts songs into the model's windows as the reference's preprocessing does (preprocess.py:165-205) and
`NoteBatch.join` puts windows behind each other again (csrc/splice.hip); `encode_song` and `vary_song` take a whole song through
the VAE on them.  `score_graph` and `score_notes` give the log-likelihood of pieces under the decoder per bar and track
(`NoteScores`, csrc/score.hip).  `Harmony` (pitch-class sets per bar and segment, `harmony=` of the generation calls) makes the
chords follow a progression, and `NoteBatch.chroma` / `NoteBatch.harmony` read the harmony of existing pieces on the device, so that
an infill can follow what the kept tracks play (csrc/sample.hip, csrc/stats.hip)."""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Any

import numpy as np
import torch

from . import ops


def generate_z(bs: int, d_model: int, device) -> torch.Tensor:
    """generate.py:90-98: a standard-normal latent batch."""
    return torch.randn(bs, d_model, device=device)


@dataclass
class ChordRules:
    """The per-track rules of chord-aware sampling (`generate_music(chord_rules=...)`, `ops.sample_chords`): `min_notes` and
    `max_notes` are an int or four ints (Drums, Bass, Guitar, Strings; 0 <= min_notes <= max_notes, 1 <= max_notes <= 14),
    `allowed_pitches` None (every pitch) or a bool array-like [4,128] whose rows `pitch_mask` helps fill."""
    min_notes: Any = 1
    max_notes: Any = 14
    allowed_pitches: Any = None


def pitch_mask(lo: int = 0, hi: int = 127, pitch_classes=None) -> np.ndarray:
    """bool [128]: the MIDI pitches lo..hi (inclusive) whose pitch class (pitch mod 12) is in `pitch_classes` (None = all):
    one track's row of `ChordRules.allowed_pitches` (a range and a scale)."""
    p = np.arange(128)
    m = (p >= lo) & (p <= hi)
    if pitch_classes is not None:
        m &= np.isin(p % 12, np.asarray(list(pitch_classes), dtype=np.int64) % 12)
    return m


@dataclass
class StructureRules:
    """The per-track rules of structure sampling (`generate_music(structure_rules=...)`, `ops.sample_structure`): one
    `temperature` (finite, >= 0; 0 = no noise), `threshold` a number or four numbers in (0, 1) (Drums, Bass, Guitar,
    Strings), `min_active` and `max_active` an int or four ints (0 <= min_active <= max_active <= 32; max_active 0 mutes the
    track), `allowed_steps` None (every step) or a bool array-like [4,32] whose rows `step_mask` helps fill."""
    temperature: Any = 1.0
    threshold: Any = 0.5
    min_active: Any = 0
    max_active: Any = 32
    allowed_steps: Any = None


def step_mask(every: int = 1, offset: int = 0, lo: int = 0, hi: int = 31) -> np.ndarray:
    """bool [32]: the timesteps lo..hi (inclusive) of a bar that lie on the grid offset, offset + every, ...: one track's row
    of `StructureRules.allowed_steps` (a grid and a window)."""
    if int(every) < 1:
        raise ValueError(f"every must be an int >= 1, got {every!r}")
    t = np.arange(32)
    return (t >= lo) & (t <= hi) & (t >= offset) & ((t - offset) % int(every) == 0)


MAJOR_SCALE = (0, 2, 4, 5, 7, 9, 11)
MINOR_SCALE = (0, 2, 3, 5, 7, 8, 10)                             # the natural minor
CHORD_QUALITIES = {"": (0, 4, 7), "m": (0, 3, 7), "7": (0, 4, 7, 10), "maj7": (0, 4, 7, 11), "m7": (0, 3, 7, 10),
                   "dim": (0, 3, 6), "aug": (0, 4, 8), "sus2": (0, 2, 7), "sus4": (0, 5, 7), "5": (0, 7)}
FREE_SET = 0xFFF                                                 # every pitch class: no constraint
_ROOTS = {"C": 0, "D": 2, "E": 4, "F": 5, "G": 7, "A": 9, "B": 11}
_SYMBOL = re.compile(r"^([A-G])([#b]?)(maj7|m7|m|7|dim|aug|sus2|sus4|5|)$")


def _set_of(root: int, intervals) -> int:
    return sum(1 << ((root + k) % 12) for k in intervals)


class Harmony:
    """A chord progression as pitch-class sets per cell (`harmony=` of `generate_music`, `generate_notes`, `vary_notes`,
    `infill_notes`, `vary_song` and, through its keywords, `pick_takes`; `ops.sample_chords_at`).  `sets` is an int tensor or
    array-like [n_bars,S] (shared by all pieces) or [B,n_bars,S]: S in {1, 2, 4, 8, 16, 32} sets per bar, each lasting 32 / S
    steps, values in [0, 4096) with bit c set = pitch class c (0 = C) may be drawn.  `tracks` (names from TRACKS or indices
    0..3) are the tracks the sets bind; the drums are left alone by default.  `empty="free"` turns a set of 0 into "no
    constraint" (0xfff), `"rest"` keeps it: the bound tracks then draw no note there.  The sets bind the onsets of the drawn
    notes; a note held into the next segment is not cut.  Bad arguments raise ValueError before a device is touched (the
    values of a device tensor are not read: bits above 11 are ignored).  `from_chords` parses chord symbols and
    `NoteBatch.harmony` reads the sets of existing pieces."""

    def __init__(self, sets, tracks=("Bass", "Guitar", "Strings"), empty="free"):
        self.sets, self.track_bits = ops.check_harmony_args(sets, tracks, empty)
        self.tracks, self.empty = tuple(tracks), empty

    def __repr__(self):
        return f"Harmony(sets={tuple(self.sets.shape)} on {self.sets.device}, tracks={self.tracks!r}, empty={self.empty!r})"

    @property
    def n_bars(self) -> int:
        return int(self.sets.shape[-2])

    @property
    def per_bar(self) -> int:
        return int(self.sets.shape[-1])

    @classmethod
    def from_chords(cls, symbols, n_bars: int, per_bar: int = 1, scale=None, tracks=("Bass", "Guitar", "Strings"),
                    empty="free") -> "Harmony":
        """The sets of chord symbols, parsed on the host: `symbols` is a list of `n_bars * per_bar` strings (`per_bar` in
        {1, 2, 4, 8, 16, 32} chords per bar, each lasting 32 / per_bar steps), a root A..G with an optional # or b and one
        of the qualities "" (major), m, 7, maj7, m7, dim, aug, sus2, sus4, 5; "N" is no chord: every pitch class (0xfff).
        With `scale="major"` or `"minor"` (natural) a symbol gives the seven-note scale on its root instead of its chord
        tones.  Raises ValueError naming a symbol it cannot read."""
        if not (ops._integer(n_bars) and n_bars >= 1):
            raise ValueError(f"n_bars must be an int >= 1, got {n_bars!r}")
        if not (ops._integer(per_bar) and per_bar in ops.SEG_STEPS):
            raise ValueError(f"per_bar must be one of {ops.SEG_STEPS}, got {per_bar!r}")
        if scale not in (None, "major", "minor"):
            raise ValueError(f"scale must be None, 'major' or 'minor', got {scale!r}")
        if isinstance(symbols, (str, bytes)) or not isinstance(symbols, (list, tuple)):
            raise ValueError(f"symbols must be a list of chord symbols, got {symbols!r}")
        if len(symbols) != n_bars * per_bar:
            raise ValueError(f"symbols must hold n_bars * per_bar = {n_bars * per_bar} chords, got {len(symbols)}")
        out = []
        for sym in symbols:
            m = _SYMBOL.match(sym) if isinstance(sym, str) else None
            if sym == "N":
                out.append(FREE_SET)
            elif m is None:
                raise ValueError(f"cannot read the chord symbol {sym!r}: a root A..G, an optional # or b and one of "
                                 f"{sorted(CHORD_QUALITIES)}, or 'N'")
            else:
                root = (_ROOTS[m.group(1)] + {"": 0, "#": 1, "b": -1}[m.group(2)]) % 12
                steps = CHORD_QUALITIES[m.group(3)] if scale is None else (MAJOR_SCALE if scale == "major" else MINOR_SCALE)
                out.append(_set_of(root, steps))
        return cls(np.asarray(out, np.int64).reshape(int(n_bars), int(per_bar)), tracks, empty)

    def check_fit(self, B: int, n_bars: int) -> None:
        """ValueError unless the sets fit a call on B pieces of n_bars bars."""
        ops.check_harmony_args(self.sets, self.tracks, self.empty, B=B, n_bars=n_bars)

    def chart(self, B: int, n_bars: int, device) -> torch.Tensor:
        """The sets as the int32 [B * n_bars, 32] chart `ops.sample_chords_at` reads (a set per step of every bar), built
        with torch ops on `device`: no host read."""
        self.check_fit(B, n_bars)
        s = self.sets.to(device).to(torch.int32) & FREE_SET
        if self.empty == "free":
            s = torch.where(s == 0, torch.full_like(s, FREE_SET), s)
        s = s.repeat_interleave(32 // self.per_bar, dim=-1)
        if s.dim() == 2:
            s = s.unsqueeze(0).expand(B, n_bars, 32)
        return s.reshape(B * n_bars, 32).contiguous()

    def _like(self, sets) -> "Harmony":
        return Harmony(sets, self.tracks, self.empty)

    def repeated(self, takes: int) -> "Harmony":
        """The harmony of `z.repeat_interleave(takes, 0)`: sets per piece are repeated per take, shared sets stay."""
        return self if self.sets.dim() == 2 else self._like(self.sets.repeat_interleave(int(takes), 0))

    def windows(self, B: int, W: int) -> "Harmony":
        """A harmony over the bars of B songs cut into the ceil(n_bars / W) windows of W bars `vary_song` decodes, [B * S, W,
        per_bar] in its order (the windows of a song behind each other); the last window is padded with free sets."""
        S = -(-self.n_bars // W)
        s = self.sets if self.sets.dim() == 3 else self.sets.unsqueeze(0).expand(B, -1, -1)
        pad = s.new_full((B, S * W - self.n_bars, self.per_bar), FREE_SET)
        if self.empty == "free":                                 # (a set of 0 stays what it is under "rest" only)
            s = torch.where(s == 0, torch.full_like(s, FREE_SET), s)
        return self._like(torch.cat([s, pad], 1).reshape(B * S, W, self.per_bar))


def _check_harmony(harmony, chord_rules, B, n_bars):
    """The checks of `harmony=` before the model is touched; returns the chord rules of the call: a harmony selects
    chord-aware sampling, so without `chord_rules` it means `ChordRules()`."""
    if harmony is None:
        return chord_rules
    if not isinstance(harmony, Harmony):
        raise ValueError(f"harmony must be a Harmony, got {harmony!r}")
    harmony.check_fit(B, n_bars)
    return ChordRules() if chord_rules is None else chord_rules


def _model_structure(vae, z, rules, seed):
    """the model's own structure for z, bool [B,n_bars,4,32]: drawn on the device from the structure logits under `rules` (a
    StructureRules) and `seed`, or, without rules, thresholded as `Decoder.forward` does it"""
    with torch.no_grad():
        s_logits = vae.engine.structure_only(z.contiguous().float(), vae.training)
    s_logits = s_logits.detach().contiguous().float()
    if rules is None:
        return vae.decoder._binary_from_logits(s_logits)
    return ops.sample_structure(s_logits, rules.temperature, rules.threshold, rules.min_active, rules.max_active,
                                rules.allowed_steps, seed)


def _decode(vae, z, s_cond, s_tensor_cond, rules=None, seed=None):
    """the decoder pass of `generate_music`: (c_logits [N,15,230] fp32, s_tensor).  With `rules` (a StructureRules) the
    structure is drawn from the structure logits on the device under `seed` and the content decoder runs on its bar graphs."""
    vae.decoder.__dict__.pop("_last_structure", None)
    if rules is not None:
        s_tensor = _model_structure(vae, z, rules, seed)
        graph = vae.decoder._structure_from_binary(s_tensor)     # (no bar is empty: s_tensor stays as drawn)
        _, c_logits = vae.decoder(z, graph)
        return c_logits.detach().contiguous().float(), s_tensor
    s_logits, c_logits = vae.decoder(z, s_cond)
    if s_tensor_cond is not None:
        s_tensor = s_tensor_cond
    elif s_cond is None:                 # the structure the decoder itself thresholded and built its graphs from
        s_tensor = vae.decoder.__dict__["_last_structure"].view(s_logits.shape).bool()
    else:
        s_tensor = vae.decoder._binary_from_logits(s_logits)
    return c_logits.detach().contiguous().float(), s_tensor


def generate_music(vae, z, s_cond=None, s_tensor_cond=None, *, temperature=None, top_k=None, top_p=None, seed=None,
                   return_tokens=False, chord_rules=None, return_note_counts=False, structure_rules=None, harmony=None):
    """generate.py:21-37.  `s_cond` is a batch of bar graphs (`vae.decoder._structure_from_binary`) or None (the
    structure then comes from the decoder's own thresholded logits); `s_tensor_cond` [B,n_bars,4,32] is the binary
    structure the pianoroll is laid out on when given.  Returns (mtp [B,n_bars,4,32,15,230], s_tensor bool).

    With `temperature`, `top_k` and `top_p` all None this is the reference's call: the active cells of `mtp` hold the
    content logits, of which `muspy_from_mtp` takes the arg-max.  With any of them given the pitch and the duration token
    of every (node, slot) are drawn on the device (`ops.sample_tokens`; `temperature` defaults to 1.0, 0 = arg-max) and the
    active cells hold their one-hot rows, so `muspy_from_mtp` decodes the drawn piece unchanged.  `seed` in [0, 2^32)
    makes the draw a pure function of the logits; None takes one from torch's CPU generator (`torch.manual_seed`
    repeats a run; no device synchronisation).  `return_tokens` appends the int32 [N,15,2] tokens (pitch, duration) to
    the returned tuple; without sampling they are the arg-max tokens of the logits `mtp` holds.

    With `chord_rules` (a `ChordRules`) the call samples chord by chord (`ops.sample_chords`: notes, one EOS, then PAD; no
    pitch twice in a chord; per-track note counts and allowed pitches), so `muspy_from_mtp` reads exactly the drawn notes.
    `temperature` defaults to 1.0 and may be a pair (pitch, duration); 0 = arg-max under the rules.  `return_note_counts`
    appends the int32 [N] note counts behind the tokens.  Bad rules raise before the model is touched.

    With `structure_rules` (a `StructureRules`; needs `s_cond` and `s_tensor_cond` both None) the structure itself is drawn
    on the device from the model's structure logits (`ops.sample_structure`: per-track threshold, least and most active
    cells, allowed steps) instead of thresholded: the content decoder runs on the drawn structure, the pianoroll is laid out
    on it and it is the `s_tensor` returned.  It combines with every content mode above.  One `seed` drives both levels
    (None draws one, once); the bars are numbered along the batch, so a `z` that repeats one latent gives several takes
    with different rhythms.  No host read is added to the one that sizes the bar graphs.

    With `harmony` (a `Harmony`: pitch-class sets per bar and segment, for all pieces or per piece) the chords follow a
    progression: the call samples chord by chord as with `chord_rules` (None then means `ChordRules()`), and a pitch of a
    track the harmony binds must also have its class in the set of its cell (`ops.sample_chords_at`).  It combines with
    every mode above.  A harmony that does not fit z's B or the model's n_bars raises before the model is touched."""
    tokens, s_tensor, note_count, c_logits = _decode_and_draw(vae, z, s_cond, s_tensor_cond, temperature, top_k, top_p, seed,
                                                              chord_rules, structure_rules, return_note_counts, return_tokens,
                                                              harmony)
    if c_logits is not None:                                     # the reference's call: the active cells hold the logits
        mtp = ops.mtp_from_logits(c_logits, s_tensor)
    else:
        mtp = ops.mtp_from_tokens(tokens, s_tensor)              # its check is the call's one host read
    out = (mtp, s_tensor)
    if return_tokens:
        out += (tokens,)
    if return_note_counts:
        out += (note_count,)
    return out


def _decode_and_draw(vae, z, s_cond, s_tensor_cond, temperature, top_k, top_p, seed, chord_rules, structure_rules,
                     return_note_counts=False, argmax_tokens=True, harmony=None):
    """The part `generate_music` and `generate_notes` share: the argument checks, the seed, the decoder pass and the draw.
    Returns (tokens int32 [N,15,2], s_tensor, note_count int32 [N] or None without chord rules, c_logits): c_logits is None
    in every sampled mode; in the unsampled one it holds the content logits and `tokens` their arg-max (None when
    `argmax_tokens` is off: the caller lays the logits out and wants no tokens)."""
    if harmony is not None:
        chord_rules = _check_harmony(harmony, chord_rules, z.shape[0], vae.cfg["n_bars"])
    sampled = _check_draw(s_cond, s_tensor_cond, temperature, top_k, top_p, seed, chord_rules, structure_rules, return_note_counts)
    if structure_rules is not None and seed is None:             # one seed for both levels, drawn before the structure
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())
    c_logits, s_tensor = _decode(vae, z, s_cond, s_tensor_cond, structure_rules, seed)
    tokens, note_count, c_logits = _draw(c_logits, s_tensor, sampled, temperature, top_k, top_p, seed, chord_rules, argmax_tokens,
                                         harmony)
    return tokens, s_tensor, note_count, c_logits


def _check_draw(s_cond, s_tensor_cond, temperature, top_k, top_p, seed, chord_rules, structure_rules, return_note_counts=False):
    """The argument checks of `_decode_and_draw`, before the model is touched.  Returns whether the content is sampled."""
    if structure_rules is not None:
        if not isinstance(structure_rules, StructureRules):
            raise ValueError(f"structure_rules must be a StructureRules, got {structure_rules!r}")
        if s_cond is not None or s_tensor_cond is not None:
            raise ValueError("structure_rules draws the structure itself: it needs s_cond and s_tensor_cond both None")
        ops.check_structure_args(structure_rules.temperature, structure_rules.threshold, structure_rules.min_active,
                                 structure_rules.max_active, structure_rules.allowed_steps, seed)
    if chord_rules is not None:
        if not isinstance(chord_rules, ChordRules):
            raise ValueError(f"chord_rules must be a ChordRules, got {chord_rules!r}")
        ops.check_chord_args(temperature, top_k, top_p, seed, chord_rules.min_notes, chord_rules.max_notes,
                             chord_rules.allowed_pitches)
        return True
    if return_note_counts:
        raise ValueError("return_note_counts needs chord_rules")
    ops.check_sampling_args(temperature, top_k, top_p, seed)
    return temperature is not None or top_k is not None or top_p is not None


def _draw(c_logits, s_tensor, sampled, temperature, top_k, top_p, seed, chord_rules, argmax_tokens=True, harmony=None):
    """The draw of `_decode_and_draw` on the content logits of the nodes of `s_tensor`, in the mode `_check_draw` found:
    (tokens, note_count, c_logits) as `_decode_and_draw` returns them.  A `seed` of None is drawn here.  With `harmony` (a
    checked Harmony; `chord_rules` is then set) the chords are drawn under its chart on s_tensor [B,n_bars,4,32]."""
    if not sampled:
        return (ops.sample_tokens(c_logits, temperature=0.0) if argmax_tokens else None), None, c_logits
    if seed is None:
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())
    if chord_rules is None:
        return ops.sample_tokens(c_logits, 1.0 if temperature is None else temperature, top_k, top_p, seed), None, None
    if harmony is not None:
        cells = ops.node_cells(s_tensor, c_logits.shape[0], check=False)
        chart = harmony.chart(s_tensor.shape[0], s_tensor.shape[1], c_logits.device)
        tokens, note_count = ops.sample_chords_at(c_logits, cells, chart, harmony.track_bits,
                                                  1.0 if temperature is None else temperature, top_k, top_p, seed,
                                                  chord_rules.min_notes, chord_rules.max_notes, chord_rules.allowed_pitches)
        return tokens, note_count, None
    track = ops.node_tracks(s_tensor, c_logits.shape[0], check=False)
    tokens, note_count = ops.sample_chords(c_logits, track, 1.0 if temperature is None else temperature, top_k, top_p, seed,
                                           chord_rules.min_notes, chord_rules.max_notes, chord_rules.allowed_pitches)
    return tokens, note_count, None


TRACKS = ("Drums", "Bass", "Guitar", "Strings")                 # constants.py:5


@dataclass
class NoteBatch:
    """A batch of generated pieces as note events on the device (`generate_notes`, `ops.notes_from_tokens`): `notes` int32
    [15 N,3] rows (time, pitch, duration) in steps of a 1 / `resolution` beat, `track_ptr` int32 [4B+1] (the rows of piece i,
    track k are notes[track_ptr[4i+k]:track_ptr[4i+k+1]], by time, then by slot), `totals` int32 [2] (notes M, active cells);
    rows from M on are not written.  A piece is `n_bars` bars of 32 steps."""
    notes: torch.Tensor
    track_ptr: torch.Tensor
    totals: torch.Tensor
    n_bars: int
    resolution: int = 8

    def tolist(self):
        """One host synchronisation: per piece, four lists (Drums, Bass, Guitar, Strings) of (time, pitch, duration)."""
        ptr = self.track_ptr.cpu().tolist()
        rows = list(zip(*self.notes[:ptr[-1]].cpu().t().tolist()))          # (time, pitch, duration) tuples of Python ints
        return [[rows[ptr[4 * i + k]:ptr[4 * i + k + 1]] for k in range(4)] for i in range((len(ptr) - 1) // 4)]

    def looped(self, n_loops: int):
        """`loop_muspy_music` (utils.py:144-160) on the lists of `tolist()`: behind every track's notes come its copies
        r = 1 .. n_loops - 1, each `r * 32 * n_bars` steps later."""
        span = 32 * self.n_bars
        return [[track + [(t + r * span, p, d) for r in range(1, int(n_loops)) for (t, p, d) in track] for track in piece]
                for piece in self.tolist()]

    def to_muspy(self, i: int, programs):
        """The `muspy.Music` the reference's `muspy_from_mtp` (utils.py:126-141) builds for piece `i`: four tracks named as
        TRACKS, Drums the drum track with program 0, the others with `programs[name]` (the caller's
        `generation_config.MIDI_PROGRAMS`), velocity 64."""
        try:
            import muspy
        except ImportError as e:
            raise ImportError("NoteBatch.to_muspy needs the muspy package (`pip install muspy`); tolist() and looped() give "
                              "the same notes as plain tuples without it") from e
        piece = self.tolist()[i]
        tracks = []
        for name, rows in zip(TRACKS, piece):
            is_drum = name == "Drums"
            tracks.append(muspy.Track(name=name, is_drum=is_drum, program=0 if is_drum else programs[name],
                                      notes=[muspy.Note(t, p, d, 64) for (t, p, d) in rows]))
        return muspy.Music(tracks=tracks, metadata=muspy.Metadata(), resolution=self.resolution)

    @classmethod
    def from_lists(cls, pieces, n_bars: int, device="cuda", resolution: int = 8) -> "NoteBatch":
        """The inverse of `tolist()`: `pieces` holds, per piece, four lists (Drums, Bass, Guitar, Strings) of (time, pitch,
        duration) ints, times in steps of a 1 / `resolution` beat inside [0, 32 n_bars).  Every track is stable-sorted by
        time on the host, so the list order of the notes of one timestep is kept: it decides which slots they take, and past
        the 14th which are dropped (the reference's "lowest position available", preprocess.py:131-144).  Raises ValueError,
        before the device is touched, on a piece without exactly four tracks, a row that is not three ints or a time outside
        the piece.  `totals` holds the notes M and the distinct (piece, track, time) cells."""
        if not (ops._integer(n_bars) and n_bars >= 1):
            raise ValueError(f"n_bars must be an int >= 1, got {n_bars!r}")
        if not isinstance(pieces, (list, tuple)) or len(pieces) == 0:
            raise ValueError("pieces must be a non-empty list of pieces")
        rows, track_ptr, cells, lim = [], [0], 0, 1 << 31
        for i, piece in enumerate(pieces):
            if not isinstance(piece, (list, tuple)) or len(piece) != 4 or not all(isinstance(t, (list, tuple)) for t in piece):
                raise ValueError(f"piece {i} must be four lists of notes (Drums, Bass, Guitar, Strings)")
            for k, track in enumerate(piece):
                for r in track:
                    if not isinstance(r, (list, tuple)) or len(r) != 3 or not all(ops._integer(v) and -lim <= v < lim for v in r):
                        raise ValueError(f"piece {i}, track {TRACKS[k]}: a note must be three ints (time, pitch, duration), got {r!r}")
                    if not 0 <= r[0] < 32 * n_bars:
                        raise ValueError(f"piece {i}, track {TRACKS[k]}: time {r[0]} is outside the piece [0, {32 * n_bars})")
                rows.extend(sorted((tuple(int(v) for v in r) for r in track), key=lambda r: r[0]))
                cells += len({r[0] for r in track})
                track_ptr.append(len(rows))
        notes = torch.from_numpy(np.asarray(rows, np.int32).reshape(-1, 3))
        return cls(notes.to(device), torch.tensor(track_ptr, dtype=torch.int32).to(device),
                   torch.tensor([len(rows), cells], dtype=torch.int32).to(device), int(n_bars), int(resolution))

    def to_graph(self):
        """The pieces as the `BarGraphBatch` the encoder consumes (`graphs.device_batch_from_notes`): two host reads."""
        from .graphs import device_batch_from_notes
        return device_batch_from_notes(self.notes, self.track_ptr, self.n_bars)

    def stats(self, check: bool = False) -> "NoteStats":
        """What the pieces hold, counted per (piece, track) on the device (`ops.note_stats`, csrc/stats.hip): one launch and
        no host read, unless `check` asks for rows outside the piece to raise."""
        track, pitch_class, onsets, sounding = ops.note_stats(self.notes, self.track_ptr, self.n_bars, check)
        B = track.shape[0] // 4
        return NoteStats(track.view(B, 4, -1), pitch_class.view(B, 4, 12), onsets.view(B, 4, -1), sounding.view(B, 4, -1),
                         self.n_bars, self.resolution)

    def chroma(self, seg_steps: int = 32) -> torch.Tensor:
        """The chromagram of the pieces, int32 [B,4,S,12] with S = 32 n_bars / `seg_steps` (1, 2, 4, 8, 16 or 32 steps per
        segment): how many (note, step) pairs of every pitch class sound in each segment of each track, notes read as
        `stats()` reads them (`ops.note_chroma`, csrc/stats.hip).  One launch, no host read."""
        c = ops.note_chroma(self.notes, self.track_ptr, self.n_bars, seg_steps)
        return c.view(c.shape[0] // 4, 4, c.shape[1], 12)

    def harmony(self, seg_steps: int = 32, tracks=("Bass", "Guitar", "Strings"), snap=None) -> "Harmony":
        """The harmony the pieces play, as a `Harmony` with sets [B,n_bars,32 / seg_steps]: the pitch classes sounding in
        `tracks` (names from TRACKS or indices 0..3) in every segment of `seg_steps` steps, from `chroma()` with torch ops on
        the device (no host read).  A segment in which those tracks are silent has the set 0, which the default
        `empty="free"` of the result reads as no constraint.  `snap="triad"` replaces every other set by the best of the 24
        major and minor triads: the chroma weight inside the triad minus the weight outside it, ties to the lowest template
        (the major triads on C..B, then the minor ones).  The result binds Bass, Guitar and Strings, whatever `tracks` it was
        read from: `Harmony(h.sets, tracks=..., empty=...)` binds otherwise."""
        if snap not in (None, "triad"):
            raise ValueError(f"snap must be None or 'triad', got {snap!r}")
        _, bits = ops.check_harmony_args(np.zeros((1, 1), np.int64), tracks)
        c = self.chroma(seg_steps).to(torch.int64)                                    # [B,4,S,12]
        dev = c.device
        use = torch.tensor([(bits >> k) & 1 for k in range(4)], dtype=torch.int64).to(dev)
        w = (c * use.view(1, 4, 1, 1)).sum(1)                                         # [B,S,12]
        sets = ((w > 0).to(torch.int64) << torch.arange(12, dtype=torch.int64, device=dev)).sum(-1)
        if snap == "triad":
            triads = [_set_of(r, CHORD_QUALITIES[q]) for q in ("", "m") for r in range(12)]
            inside = torch.tensor([[(t >> k) & 1 for k in range(12)] for t in triads], dtype=torch.int64).to(dev)       # [24,12]
            score = 2 * (w.unsqueeze(-2) * inside).sum(-1) - w.sum(-1, keepdim=True)                                  # [B,S,24]
            best = (score * 24 + torch.arange(23, -1, -1, dtype=torch.int64, device=dev)).argmax(-1)                  # (distinct keys)
            sets = torch.where(sets > 0, torch.tensor(triads, dtype=torch.int64).to(dev)[best], sets)
        return Harmony(sets.view(c.shape[0], self.n_bars, 32 // int(seg_steps)))

    def select(self, index, check: bool = True) -> "NoteBatch":
        """The pieces `index[0..K)` (an int32 or int64 tensor or a list; entries in [0, B), distinct) as a NoteBatch of their
        own, in that order, copied on the device (`ops.notes_select`).  `check` costs one host read and raises ValueError on
        an entry out of range or repeated; without it such an entry gives an empty piece.  `totals[1]` counts the cells as
        `from_lists` does (the distinct (piece, track, time) of sorted tracks), not the model's active cells."""
        notes, track_ptr, totals, _ = ops.notes_select(self.notes, self.track_ptr, index, check)
        return NoteBatch(notes, track_ptr, totals, self.n_bars, self.resolution)

    def windows(self, n_bars: int, stride: int = 1, song_bars=None, filter=None, transpose=None, seed=None,
                check: bool = True):
        """Songs cut into windows of `n_bars` bars, on the device (`ops.notes_splice`, csrc/splice.hip): the reference's
        sliding window (preprocess.py:165-205).  The windows of song b start at the bars 0, `stride`, ... while
        start + n_bars <= song_bars[b], songs in order; a note goes into a window by its onset and is never cut, the order of
        a track's rows is kept.  Returns (NoteBatch of the windows, WindowIndex: which song and bar each came from, the shift
        it got).  The notes buffer holds M ceil(n_bars / stride) rows, a bound that needs no host read.
        `song_bars`: the bars of every song, at most `self.n_bars`, which is the default.  A list is read on the host, and the
        result holds exactly the windows that fit.  A tensor [B] is not read: the result then holds
        (self.n_bars - n_bars) // stride + 1 pieces per song, and those that do not fit into their song are silent and have
        `song` = -1 in the index.
        `filter="reference"` drops the windows the reference's silence rules reject (preprocess.py:176-194; n_bars <= 64):
        the rule is applied on the device, but how many windows stay sizes the result, so this is the one place where a host
        read is inherent.  ValueError when none stays.
        `transpose`: None, an int, an int tensor [K] (a shift per window, in the order of the result before the filter), or
        "random": `torch.randint(-5, 7)` on the device from a generator seeded with `seed` (None: the device's global one),
        preprocess.py:198.  Tracks 1..3 get clamp(clamp(pitch, 0, 127) + shift, 0, 127), the drums stay.
        `check` costs one host read and raises ValueError if the kernel counted anything it did not follow."""
        if not (ops._integer(n_bars) and n_bars >= 1):
            raise ValueError(f"n_bars must be an int >= 1, got {n_bars!r}")
        if not (ops._integer(stride) and stride >= 1):
            raise ValueError(f"stride must be an int >= 1, got {stride!r}")
        if filter not in (None, "reference"):
            raise ValueError(f"filter must be None or 'reference', got {filter!r}")
        if filter is not None and n_bars > ops.MAX_RULE_BARS:
            raise ValueError(f"filter='reference' needs n_bars <= {ops.MAX_RULE_BARS}, got {n_bars}")
        ops.check_sampling_args(seed=seed)
        check_device = ops._note_batch_args(self.notes, self.track_ptr)
        if not (ops._integer(self.n_bars) and self.n_bars >= 1):
            raise ValueError(f"the batch's n_bars must be an int >= 1, got {self.n_bars!r}")
        n_bars, stride, B, M = int(n_bars), int(stride), self.track_ptr.shape[0] // 4, self.notes.shape[0]
        per = (self.n_bars - n_bars) // stride + 1 if n_bars <= self.n_bars else 0       # windows of a whole song
        counts = None                                                                 # windows per song, where the host knows
        if song_bars is None:
            counts = [per] * B
        elif isinstance(song_bars, (list, tuple)):
            if len(song_bars) != B or not all(ops._integer(v) and 0 <= v <= self.n_bars for v in song_bars):
                raise ValueError(f"song_bars must hold {B} ints in [0, {self.n_bars}], got {song_bars!r}")
            counts = [(int(v) - n_bars) // stride + 1 if v >= n_bars else 0 for v in song_bars]
        elif not (isinstance(song_bars, torch.Tensor) and song_bars.dtype in (torch.int32, torch.int64) and tuple(song_bars.shape) == (B,)):
            raise ValueError(f"song_bars must be None, a list of {B} ints or an int32 / int64 tensor [{B}], got {song_bars!r}")
        K = sum(counts) if counts is not None else B * per
        if K < 1:
            raise ValueError(f"no window of {n_bars} bars fits into songs of {self.n_bars} bars" + (f" (song_bars = {song_bars!r})" if counts else ""))
        if isinstance(transpose, torch.Tensor):
            if transpose.dtype not in (torch.int32, torch.int64) or tuple(transpose.shape) != (K,):
                raise ValueError(f"transpose must be an int tensor [K = {K}], got {transpose.dtype} {tuple(transpose.shape)}")
        elif not (transpose is None or transpose == "random" or (ops._integer(transpose) and -127 <= transpose <= 127)):
            raise ValueError(f"transpose must be None, an int in [-127, 127], an int tensor [K = {K}] or 'random', got {transpose!r}")
        check_device()
        dev = self.notes.device
        for t, name in ((song_bars, "song_bars"), (transpose, "transpose")):
            if isinstance(t, torch.Tensor) and t.device != dev:
                raise ValueError(f"{name} lives on {t.device}, notes on {dev}")
        arange = lambda n: torch.arange(n, dtype=torch.int64, device=dev)
        if counts is not None:                                   # every window fits: one segment each, in place
            if song_bars is None:
                song, start = arange(B).repeat_interleave(per), arange(per).repeat(B) * stride
            else:
                c = torch.tensor(counts, dtype=torch.int64).to(dev)
                song = torch.repeat_interleave(arange(B), c, output_size=K)
                start = (arange(K) - (c.cumsum(0) - c)[song]) * stride
            seg_ptr = arange(K + 1)
            rows = torch.stack([song, start, torch.zeros_like(song), torch.full_like(song, n_bars)], 1)
        else:                                                    # the segments of the windows that fit first, in order
            song, start = arange(B).repeat_interleave(per), arange(per).repeat(B) * stride
            fits = start + n_bars <= song_bars.to(torch.int64).clamp(0, self.n_bars)[song]
            order = torch.argsort((~fits).to(torch.int8), stable=True)
            rows = torch.stack([song, start, torch.zeros_like(song), torch.full_like(song, n_bars)], 1)[order]
            seg_ptr = torch.cat([fits.new_zeros(1, dtype=torch.int64), fits.cumsum(0)])
            song = torch.where(fits, song, torch.full_like(song, -1))
        if transpose is None:
            shift, used = None, torch.zeros(K, dtype=torch.int32, device=dev)
        elif isinstance(transpose, torch.Tensor):
            shift = used = transpose.clamp(-128, 128).to(torch.int32)
        elif transpose == "random":
            gen = None if seed is None else torch.Generator(device=dev).manual_seed(int(seed))
            shift = used = torch.randint(-5, 7, (K,), generator=gen, device=dev, dtype=torch.int32)
        else:
            shift = used = torch.full((K,), int(transpose), dtype=torch.int32, device=dev)
        cap = M * (-(-n_bars // stride))
        notes, track_ptr, totals, keep, _ = ops.notes_splice(self.notes, self.track_ptr, self.n_bars, rows.to(torch.int32),
                                                             seg_ptr.to(torch.int32), n_bars, shift, filter is not None, cap, check)
        out = NoteBatch(notes, track_ptr, totals, n_bars, self.resolution)
        index = WindowIndex(song.to(torch.int32), start.to(torch.int32), used)
        if filter is not None:
            kept = keep.nonzero().flatten()                      # the host read that sizes the result
            if kept.numel() == 0:
                raise ValueError(f"filter='reference' rejects all {K} windows")
            out = out.select(kept, check=False)
            index = WindowIndex(index.song[kept], index.start[kept], index.shift[kept])
        return out, index

    def join(self, index, hop_bars=None, check: bool = True) -> "NoteBatch":
        """Pieces put behind each other in time, on the device (`ops.notes_splice`): the inverse of `windows`.  `index` is
        int [K,G], a tensor or nested lists: output piece j is made of the pieces index[j, 0..G) of this batch, -1 standing
        for a silent window.  With W = `self.n_bars` and `hop_bars` in [1, W] (W by default) an output piece has
        hop (G - 1) + W bars: window g gives its first `hop` bars from bar g hop on, the last window all W of them.  The
        entries that are not -1 must lie in [0, B) and be distinct, which is what bounds the result by the input's rows;
        `check` costs one host read and raises ValueError otherwise.  Without it an entry out of range gives silence and
        the rows that repeated entries push beyond the buffer are not written."""
        W = self.n_bars
        hop = W if hop_bars is None else hop_bars
        if not (ops._integer(W) and W >= 1):
            raise ValueError(f"the batch's n_bars must be an int >= 1, got {W!r}")
        if not (ops._integer(hop) and 1 <= hop <= W):
            raise ValueError(f"hop_bars must be an int in [1, {W}], got {hop_bars!r}")
        check_device = ops._note_batch_args(self.notes, self.track_ptr)
        if isinstance(index, torch.Tensor):
            if index.dtype not in (torch.int32, torch.int64) or index.dim() != 2 or index.numel() == 0:
                raise ValueError(f"index must be an int32 or int64 tensor [K,G] with K, G >= 1, got {index.dtype} {tuple(index.shape)}")
        elif (isinstance(index, (list, tuple)) and len(index) >= 1 and all(isinstance(r, (list, tuple)) and len(r) >= 1 for r in index)
              and len({len(r) for r in index}) == 1 and all(ops._integer(v) and -(1 << 31) <= v < (1 << 31) for r in index for v in r)):
            index = torch.tensor([[int(v) for v in r] for r in index], dtype=torch.int64)
            if self.notes.is_cuda:
                index = index.to(self.notes.device)
        else:
            raise ValueError(f"index must be an int tensor [K,G] or K lists of G ints, K, G >= 1, got {index!r}")
        K, G = index.shape
        out_bars = int(hop) * (G - 1) + W
        if out_bars > 0x7fffffff // 32 or K * G > 0x7fffffff // 4:
            raise ValueError(f"index [{K},{G}] gives pieces of {out_bars} bars: too many")
        check_device()
        dev = self.notes.device
        if index.device != dev:
            raise ValueError(f"index lives on {index.device}, notes on {dev}")
        B = self.track_ptr.shape[0] // 4
        flat = index.reshape(-1).to(torch.int64).clamp(-2, B)    # (an entry beyond int32 is out of range either way)
        used = flat != -1
        g = torch.arange(G, dtype=torch.int64, device=dev).repeat(K)
        bars = torch.where(g == G - 1, torch.full_like(g, W), torch.full_like(g, int(hop)))
        order = torch.argsort((~used).to(torch.int8), stable=True)                   # the silent windows have no segment
        rows = torch.stack([flat, torch.zeros_like(g), g * int(hop), bars], 1)[order].to(torch.int32)
        seg_ptr = torch.cat([used.new_zeros(1, dtype=torch.int64), used.view(K, G).sum(1).cumsum(0)]).to(torch.int32)
        notes, track_ptr, totals, _, status = ops.notes_splice(self.notes, self.track_ptr, W, rows, seg_ptr, out_bars, check=False)
        if check:
            inside = (flat >= 0) & (flat < B)
            seen = torch.zeros(B + 1, dtype=torch.int64, device=dev).scatter_add_(0, torch.where(inside, flat, torch.full_like(flat, B)),
                                                                                   torch.ones_like(flat))
            repeated = (seen[:B] - 1).clamp(min=0).sum().view(1)
            outside, _, excess, _, repeated = torch.cat([status.to(torch.int64), repeated]).tolist()     # the one host read
            if outside or repeated or excess:
                raise ValueError(f"index: {outside} entries outside [0, {B}) that are not -1, {repeated} entries that repeat an "
                                 f"earlier one ({excess} rows beyond the buffer)")
        return NoteBatch(notes, track_ptr, totals, out_bars, self.resolution)


@dataclass
class WindowIndex:
    """Where the pieces `NoteBatch.windows` returned come from, int32 [K] tensors on the device, aligned with the pieces:
    `song` (the piece of the input; -1 for a window that did not fit into a song whose length was given as a tensor), `start`
    (its first bar there) and `shift` (the semitones tracks 1..3 were transposed by, 0 without `transpose`)."""
    song: torch.Tensor
    start: torch.Tensor
    shift: torch.Tensor


@dataclass
class NoteStats:
    """The counts of `NoteBatch.stats()` (`ops.note_stats`, "Note statistics" in include/polyphemus_hip.h), int32 on the
    device: `track` [B,4,12] (fields `ops.NOTE_STAT_FIELDS`: n_notes, n_onsets, pitch_min, pitch_max, n_pitches,
    n_pitch_classes, note_steps, sounding_steps, poly_steps, max_polyphony, max_chord, out_of_range), `pitch_class` [B,4,12]
    (notes per pitch mod 12), `onsets` and `sounding` [B,4,n_bars] (bit s of word b: step 32 b + s has an onset / a sounding
    note).  A note is a row whose time lies inside the piece, with the pitch clamped to 0..127 and the duration to 1..96 and
    cut at the end of the piece: what the encoder sees, which is where the measures below differ from `muspy.metrics` on
    `to_muspy()` (muspy takes pitches and durations as they are and lets the last notes sound beyond the piece).  The methods
    are torch ops on the device, float32 [B,4] unless noted, without a host read."""
    track: torch.Tensor
    pitch_class: torch.Tensor
    onsets: torch.Tensor
    sounding: torch.Tensor
    n_bars: int
    resolution: int = 8

    def field(self, name: str) -> torch.Tensor:
        """int32 [B,4]: one field of `track` by its name in `ops.NOTE_STAT_FIELDS`"""
        return self.track[..., ops.NOTE_STAT_FIELDS.index(name)]

    def polyphony(self) -> torch.Tensor:
        """`muspy.metrics.polyphony`: the mean number of notes sounding over the steps at which any sounds, note_steps /
        sounding_steps; 0 for a silent track (muspy: nan).  Durations are clamped and cut at the end of the piece."""
        num, den = self.field("note_steps").float(), self.field("sounding_steps").float()
        return torch.where(den > 0, num / den.clamp(min=1), torch.zeros_like(num))

    def polyphony_rate(self) -> torch.Tensor:
        """`muspy.metrics.polyphony_rate` with threshold 2: the share of the piece's 32 n_bars steps at which at least two
        notes sound.  muspy divides by the length up to the end of the last note; here the piece's length is fixed."""
        return self.field("poly_steps").float() / float(32 * self.n_bars)

    def pitch_class_entropy(self) -> torch.Tensor:
        """`muspy.metrics.pitch_class_entropy`: the Shannon entropy in bits of the notes' pitch-class histogram; 0 for a
        track without notes (muspy: nan).  Pitches are clamped to 0..127 first."""
        c = self.pitch_class.float()
        p = c / c.sum(-1, keepdim=True).clamp(min=1)
        return -(p * torch.log2(torch.where(p > 0, p, torch.ones_like(p)))).sum(-1)

    def scale_consistency(self) -> torch.Tensor:
        """`muspy.metrics.scale_consistency`: the largest share of notes inside one of the 12 transpositions of the major
        scale (classes 0, 2, 4, 5, 7, 9, 11; the natural minor scales are the same 12 sets, which muspy walks a second time);
        0 for a track without notes (muspy: nan)."""
        c = self.pitch_class.float()
        scales = torch.zeros(12, 12, dtype=c.dtype, device=c.device)
        for root in range(12):
            scales[root, [(root + k) % 12 for k in MAJOR_SCALE]] = 1.0
        inside = (c.unsqueeze(-2) * scales).sum(-1).amax(-1)     # (sums of small integers: exact in fp32)
        return inside / c.sum(-1).clamp(min=1)

    def groove_consistency(self) -> torch.Tensor:
        """`muspy.metrics.groove_consistency` with a measure of 32 steps: 1 minus the mean over neighbouring bars of the
        Hamming distance of their onset patterns / 32; 1 when n_bars == 1 (muspy: nan).  muspy's last measure ends with the
        last note; here every bar of the piece counts."""
        if self.n_bars == 1:
            return torch.ones(self.onsets.shape[:2], dtype=torch.float32, device=self.onsets.device)
        diff = _popcount32(self.onsets[..., :-1] ^ self.onsets[..., 1:]).float()
        return 1.0 - diff.sum(-1) / float(32 * (self.n_bars - 1))

    def empty_beat_rate(self) -> torch.Tensor:
        """`muspy.metrics.empty_beat_rate`, float32 [B]: the share of the piece's 4 n_bars beats (`resolution` steps each) in
        which no track sounds.  muspy counts a beat as used when a note starts in it and stops at the last note's end; here a
        beat is used while a note sounds in it, and all beats of the piece count."""
        r = self.resolution
        if not (ops._integer(r) and r >= 1 and 32 % r == 0):
            raise ValueError(f"resolution must divide 32 (a bar's steps), got {r!r}")
        any_track = self.sounding[:, 0] | self.sounding[:, 1] | self.sounding[:, 2] | self.sounding[:, 3]       # [B,n_bars]
        shifts = torch.arange(0, 32, r, dtype=torch.int32, device=any_track.device)
        mask = -1 if r == 32 else (1 << r) - 1
        used = ((any_track.unsqueeze(-1) >> shifts) & mask) != 0                                                # [B,n_bars,32/r]
        return 1.0 - used.float().mean(dim=(1, 2))


def _popcount32(x: torch.Tensor) -> torch.Tensor:
    """int32 -> the number of set bits of every word (the sign bit counts), by the parallel-sum identity"""
    x = x.to(torch.int64) & 0xFFFFFFFF
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) & 0xFFFFFFFF) >> 24


def pick_takes(vae, z, takes: int, key, **generate_notes_kwargs):
    """Several takes of every latent, the best of each kept by a criterion, chosen on the device.  `z` is [B,d];
    `z.repeat_interleave(takes, 0)` goes through ONE `generate_notes` call (rows that repeat a latent differ in their draws, so
    sampling or `structure_rules` is what makes takes differ), `key(stats)` gets the `NoteStats` of the B * takes pieces and
    returns a float tensor [B * takes] on their device, higher is better; NaN counts as -inf.  Of each group of `takes`
    consecutive rows the best is kept, ties go to the lowest row.  `s_cond` (bar graphs) and `s_tensor_cond` [B,n_bars,4,32],
    if given, are repeated as `z` is, and so are the sets of a `harmony` that has them per piece.  Returns (NoteBatch of B pieces, s_tensor [B,n_bars,4,32] of the winners, chosen int64 [B]:
    the row of each winner among the B * takes).  No host read beyond `generate_notes`' own."""
    if not (ops._integer(takes) and takes >= 1):
        raise ValueError(f"takes must be an int >= 1, got {takes!r}")
    if "return_tokens" in generate_notes_kwargs:
        raise ValueError("return_tokens is not an argument of pick_takes: the tokens of the takes are not kept")
    if not callable(key):
        raise ValueError(f"key must be a callable NoteStats -> float tensor [B * takes], got {key!r}")
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[0] < 1:
        raise ValueError(f"z must be a tensor [B,d] with B >= 1, got {type(z).__name__}"
                         + (f" {tuple(z.shape)}" if isinstance(z, torch.Tensor) else ""))
    takes, B = int(takes), z.shape[0]
    kw = dict(generate_notes_kwargs)
    s_cond, s_tensor_cond = kw.pop("s_cond", None), kw.pop("s_tensor_cond", None)
    if isinstance(kw.get("harmony"), Harmony):                   # sets per piece are repeated as `z` is
        kw["harmony"].check_fit(B, kw["harmony"].n_bars)
        kw["harmony"] = kw["harmony"].repeated(takes)
    if s_tensor_cond is not None:
        s_tensor_cond = s_tensor_cond.repeat_interleave(takes, 0)
    if s_cond is not None:                                       # the bar graphs of the repeated structure
        s_rep = s_cond.s_tensor.view(B, -1, 4, 32).bool().repeat_interleave(takes, 0)
        s_cond = vae.decoder._structure_from_binary(s_rep)
    batch, s_tensor = generate_notes(vae, z.repeat_interleave(takes, 0), s_cond, s_tensor_cond, **kw)
    score = key(batch.stats())
    if (not isinstance(score, torch.Tensor) or not score.is_floating_point() or tuple(score.shape) != (B * takes,)
            or score.device != batch.notes.device):
        got = f"{score.dtype} {tuple(score.shape)} on {score.device}" if isinstance(score, torch.Tensor) else type(score).__name__
        raise ValueError(f"key must return a float tensor [{B * takes}] on {batch.notes.device}, got {got}")
    score = torch.nan_to_num(score.float(), nan=float("-inf"), posinf=float("inf"), neginf=float("-inf")).view(B, takes)
    chosen = score.argmax(1) + takes * torch.arange(B, device=score.device)     # (argmax: the first of equal maxima)
    return batch.select(chosen, check=False), s_tensor[chosen], chosen


def generate_notes(vae, z, s_cond=None, s_tensor_cond=None, *, temperature=None, top_k=None, top_p=None, seed=None,
                   chord_rules=None, structure_rules=None, return_tokens=False, harmony=None):
    """`generate_music` without the pianoroll: the same arguments, checks, seed handling and draws in every mode (unsampled =
    the arg-max tokens), but the pieces come back as a `NoteBatch` — the notes the reference's `muspy_from_mtp` would read out
    of `generate_music`'s `mtp`, in its order — read from the tokens on the device (`ops.notes_from_tokens`).  Returns
    (NoteBatch, s_tensor), with `return_tokens` the int32 [N,15,2] tokens appended.  One host read beyond the one that sizes
    the bar graphs: the check that the structure has as many active cells as the decoder gave nodes."""
    tokens, s_tensor, _, _ = _decode_and_draw(vae, z, s_cond, s_tensor_cond, temperature, top_k, top_p, seed, chord_rules,
                                              structure_rules, harmony=harmony)
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, s_tensor)
    batch = NoteBatch(notes, track_ptr, totals, int(s_tensor.shape[1]))
    return (batch, s_tensor, tokens) if return_tokens else (batch, s_tensor)


def _check_batch(vae, batch):
    if not isinstance(batch, NoteBatch):
        raise ValueError(f"batch must be a NoteBatch, got {type(batch).__name__}")
    if batch.n_bars != vae.cfg["n_bars"]:
        raise ValueError(f"batch holds pieces of n_bars = {batch.n_bars}, the model takes n_bars = {vae.cfg['n_bars']}")


def _encode(vae, batch):
    """(mu, log_var, graph) of a NoteBatch: the encoder in eval mode without gradients, the mode it found restored."""
    _check_batch(vae, batch)
    graph = batch.to_graph()
    was_training = vae.training
    vae.eval()
    try:
        with torch.no_grad():
            mu, log_var = vae.encoder(graph)
    finally:
        vae.train(was_training)
    return mu, log_var, graph


def encode_notes(vae, batch):
    """The latent of pieces held as notes: (mu, log_var) [B,d] of `vae.encoder` on `batch.to_graph()` (a `NoteBatch`, from
    `generate_notes` or `NoteBatch.from_lists`), in eval mode and without gradients; `vae.training` is left as found.  Raises
    ValueError when `batch.n_bars` is not the model's."""
    return _encode(vae, batch)[:2]


def vary_notes(vae, batch, strength=1.0, keep_structure=False, seed=None, return_z=False, **generate_notes_kwargs):
    """Variations of pieces held as notes: `batch` is encoded (`encode_notes`) and `generate_notes` decodes
    z = mu + strength * exp(log_var / 2) * eps.  `eps` is drawn on the CPU from a generator seeded with `seed`, None takes
    torch's global generator; the same `seed` goes on to `generate_notes` for all its levels.  `strength` is finite and >= 0;
    0 is the reconstruction at mu.  `keep_structure` decodes on the input's own structure (its bar graphs as `s_cond`, its
    cells as `s_tensor_cond`): same rhythm, new notes; it excludes `structure_rules` with the error `generate_music` raises.
    Every other keyword is `generate_notes`', `harmony=` among them.  Returns what `generate_notes` returns, (NoteBatch,
    s_tensor[, tokens]), with `return_z` the latent appended."""
    if not (ops._real(strength) and np.isfinite(strength) and strength >= 0):
        raise ValueError(f"strength must be a finite number >= 0, got {strength!r}")
    ops.check_sampling_args(seed=seed)
    for k in ("s_cond", "s_tensor_cond"):
        if k in generate_notes_kwargs:
            raise ValueError(f"{k} is not an argument of vary_notes: keep_structure=True passes the input's structure")
    if keep_structure and generate_notes_kwargs.get("structure_rules") is not None:
        raise ValueError("structure_rules draws the structure itself: it needs s_cond and s_tensor_cond both None")
    if generate_notes_kwargs.get("harmony") is not None:         # before the encoder runs
        _check_batch(vae, batch)
        _check_harmony(generate_notes_kwargs["harmony"], None, (batch.track_ptr.shape[0] - 1) // 4, batch.n_bars)
    mu, log_var, graph = _encode(vae, batch)
    z = mu
    if strength != 0:
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        eps = torch.randn(mu.shape, generator=gen, dtype=torch.float32).to(mu.device)
        z = mu + float(strength) * torch.exp(0.5 * log_var) * eps
    s_cond = s_tensor_cond = None
    if keep_structure:
        s_cond, s_tensor_cond = graph, graph.s_tensor.view(-1, batch.n_bars, 4, 32).bool()
    out = generate_notes(vae, z, s_cond, s_tensor_cond, seed=seed, **generate_notes_kwargs)
    return out + (z,) if return_z else out


def _song_windows(vae, song):
    """(the windows of `song` as a NoteBatch of the model's n_bars = W, B, windows per song S): W bars each, one behind the
    other.  A song whose length is no multiple of W counts as padded with silence up to the next one: `n_bars` is a label on
    the layout, so the padding moves nothing.  No host read."""
    if not isinstance(song, NoteBatch):
        raise ValueError(f"song must be a NoteBatch, got {type(song).__name__}")
    W = vae.cfg["n_bars"]
    if not (ops._integer(song.n_bars) and song.n_bars >= 1):
        raise ValueError(f"song.n_bars must be an int >= 1, got {song.n_bars!r}")
    S = -(-song.n_bars // W)
    padded = NoteBatch(song.notes, song.track_ptr, song.totals, S * W, song.resolution)
    wins, _ = padded.windows(W, stride=W, check=False)
    return wins, song.track_ptr.shape[0] // 4, S


def encode_song(vae, song):
    """The latents of whole songs: `song` (a `NoteBatch` of B songs of any length) is cut into the S = ceil(n_bars / W)
    windows of the model's W bars on the device (`NoteBatch.windows(W, stride=W)`) and every window is encoded
    (`encode_notes`).  Returns (mu, log_var) [B,S,d].  A last window that the song fills only partly is silent behind the
    song's end."""
    wins, B, S = _song_windows(vae, song)
    mu, log_var = encode_notes(vae, wins)
    return mu.reshape(B, S, -1), log_var.reshape(B, S, -1)


def vary_song(vae, song, strength=1.0, keep_structure=False, seed=None, **generate_notes_kwargs):
    """Variations of whole songs: `song` is cut into windows of the model's W bars, the windows go through `vary_notes`
    as one batch (its arguments, `strength=0` is the reconstruction) and come back behind each other (`NoteBatch.join`) as a
    NoteBatch of B songs of W ceil(n_bars / W) bars.  Cutting and joining happen on the device and read nothing back, so
    the host reads are those of `vary_notes`.  A `harmony=` spans the song's bars ([n_bars,S] or [B,n_bars,S] with the song's
    n_bars) and is cut into the windows with it; the bars a last window has beyond the song's end are free."""
    for k in ("return_tokens", "return_z"):
        if k in generate_notes_kwargs:
            raise ValueError(f"{k} is not an argument of vary_song: the windows' tokens and latents are not kept")
    if not isinstance(song, NoteBatch):
        raise ValueError(f"song must be a NoteBatch, got {type(song).__name__}")
    if not (ops._real(strength) and np.isfinite(strength) and strength >= 0):
        raise ValueError(f"strength must be a finite number >= 0, got {strength!r}")
    kw = dict(generate_notes_kwargs)
    if kw.get("harmony") is not None:                            # over the song's bars: cut into the windows
        h = kw["harmony"]
        if not (ops._integer(song.n_bars) and song.n_bars >= 1):
            raise ValueError(f"song.n_bars must be an int >= 1, got {song.n_bars!r}")
        _check_harmony(h, None, (song.track_ptr.shape[0] - 1) // 4, song.n_bars)
        kw["harmony"] = h.windows((song.track_ptr.shape[0] - 1) // 4, vae.cfg["n_bars"])
    wins, B, S = _song_windows(vae, song)
    varied = vary_notes(vae, wins, strength, keep_structure, seed, **kw)[0]
    index = torch.arange(B * S, dtype=torch.int32, device=varied.notes.device).view(B, S)
    return varied.join(index, check=False)


def region_mask(n_bars: int, tracks=None, bars=None, steps=None) -> np.ndarray:
    """bool [n_bars,4,32]: the region of an infill (`infill_notes`), True = the model rewrites the cell.  `tracks` holds names
    from TRACKS or indices 0..3, `bars` indices 0..n_bars-1, `steps` is a bool [32] array as `step_mask` returns; None means
    all, and the three are ANDed together.  Bad values raise ValueError naming the argument."""
    if not (ops._integer(n_bars) and n_bars >= 1):
        raise ValueError(f"n_bars must be an int >= 1, got {n_bars!r}")
    on_track, on_bar, on_step = np.ones(4, bool), np.ones(int(n_bars), bool), np.ones(32, bool)
    if tracks is not None:
        if isinstance(tracks, (str, bytes)) or not isinstance(tracks, (list, tuple, set, frozenset, np.ndarray)):
            raise ValueError(f"tracks must be a list of names from {TRACKS} or indices 0..3, got {tracks!r}")
        on_track[:] = False
        for k in tracks:
            if isinstance(k, str) and k in TRACKS:
                k = TRACKS.index(k)
            if not (ops._integer(k) and 0 <= k < 4):
                raise ValueError(f"tracks must hold names from {TRACKS} or indices 0..3, got {k!r}")
            on_track[int(k)] = True
    if bars is not None:
        if not isinstance(bars, (list, tuple, set, frozenset, range, np.ndarray)):
            raise ValueError(f"bars must be a list of indices 0..{n_bars - 1}, got {bars!r}")
        on_bar[:] = False
        for b in bars:
            if not (ops._integer(b) and 0 <= b < n_bars):
                raise ValueError(f"bars must hold indices 0..{n_bars - 1}, got {b!r}")
            on_bar[int(b)] = True
    if steps is not None:
        a = steps.detach().cpu().numpy() if isinstance(steps, torch.Tensor) else np.asarray(steps)
        if a.dtype != np.bool_ or a.shape != (32,):
            raise ValueError(f"steps must be a bool array of shape [32], got {a.dtype} {tuple(a.shape)}")
        on_step = a
    return np.ascontiguousarray(on_bar[:, None, None] & on_track[None, :, None] & on_step[None, None, :])


def infill_notes(vae, batch, region, strength=0.0, keep_structure=False, seed=None, return_z=False, return_info=False,
                 **generate_notes_kwargs):
    """Regenerate part of pieces held as notes and keep the rest: `region` (bool [n_bars,4,32] for all pieces or
    [B,n_bars,4,32], see `region_mask`; True = the model rewrites the cell) says which (bar, track, step) cells are written
    anew, every other cell comes back with the notes the encoder saw.  `batch` (a `NoteBatch`, checked as by `encode_notes`)
    is encoded once and the fill is decoded at z = mu + strength * exp(log_var / 2) * eps, `eps` and `seed` handled as in
    `vary_notes`; the default `strength` 0 decodes at the piece's own latent.

    Structure: the model's structure for z is thresholded, or drawn under `structure_rules=` (the draw `generate_notes`
    makes), and merged with the input's on the device (`ops.infill_structure`): a cell is on iff (region ? model : input), a
    bar that comes out empty gets cell [0,0].  The per-track bounds of `structure_rules` hold for the model's structure: inside
    a region that covers only part of a track just `max_active` is guaranteed, `min_active` cells may fall outside it.  With
    `keep_structure=True` the merged structure is the input's own and only the notes inside the region change; it excludes
    `structure_rules` with the error `vary_notes` raises.

    Decoding: the content decoder runs on the merged structure's bar graphs and the tokens of every node are drawn in the
    mode the keywords select, with `generate_notes`' arguments and checks (unsampled = arg-max, `temperature` / `top_k` /
    `top_p`, `chord_rules`, `harmony`); `ops.infill_tokens` puts the kept cells' tokens back and `ops.notes_from_tokens` reads the
    piece, so a harmony acts on the region only: `harmony=batch.harmony(tracks=...)` makes the new part follow what the kept
    tracks play.
    The decoder is not autoregressive: given z and the bar graph the regenerated cells do not depend on the kept notes.
    `s_cond` / `s_tensor_cond` are rejected as in `vary_notes`.

    Outside the region the result holds what the encoder saw, not the raw input: pitches clamped to 0..127, durations to
    1..96, the first 14 notes of a cell, and durations cut at the piece's end by the reader.

    Returns (NoteBatch, s_tensor bool [B,n_bars,4,32]) and then, as asked, `return_tokens` the int32 [N,15,2] tokens,
    `return_z` the latent, `return_info` the int32 [5] status of `ops.infill_tokens`, left on the device (merged cells, input
    cells, kept nodes, kept nodes without a source, bars forced).  No host read beyond those of `to_graph`, the graph build
    of the merged structure and the `notes_from_tokens` check."""
    if not (ops._real(strength) and np.isfinite(strength) and strength >= 0):
        raise ValueError(f"strength must be a finite number >= 0, got {strength!r}")
    ops.check_sampling_args(seed=seed)
    kw = dict(generate_notes_kwargs)
    for k in ("s_cond", "s_tensor_cond"):
        if k in kw:
            raise ValueError(f"{k} is not an argument of infill_notes: keep_structure=True keeps the input's structure")
    temperature, top_k, top_p = kw.pop("temperature", None), kw.pop("top_k", None), kw.pop("top_p", None)
    chord_rules, structure_rules = kw.pop("chord_rules", None), kw.pop("structure_rules", None)
    return_tokens, harmony = kw.pop("return_tokens", False), kw.pop("harmony", None)
    if kw:
        raise TypeError(f"infill_notes got an unexpected keyword argument {sorted(kw)[0]!r}")
    if keep_structure and structure_rules is not None:
        raise ValueError("structure_rules draws the structure itself: it needs s_cond and s_tensor_cond both None")
    _check_batch(vae, batch)
    B, n_bars = (batch.track_ptr.shape[0] - 1) // 4, batch.n_bars
    region = ops.check_region(region, B, n_bars)
    chord_rules = _check_harmony(harmony, chord_rules, B, n_bars)
    sampled = _check_draw(None, None, temperature, top_k, top_p, seed, chord_rules, structure_rules)
    mu, log_var, graph = _encode(vae, batch)
    z = mu
    if strength != 0:
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        eps = torch.randn(mu.shape, generator=gen, dtype=torch.float32).to(mu.device)
        z = mu + float(strength) * torch.exp(0.5 * log_var) * eps
    s_in = graph.s_tensor
    region = torch.from_numpy(region.reshape(-1, 4, 32)).to(s_in.device)
    if keep_structure:
        merged, bar_forced = graph, None
    else:
        if structure_rules is not None and seed is None:         # one seed for both levels, drawn before the structure
            seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())
        s_bool, bar_forced = ops.infill_structure(s_in, _model_structure(vae, z, structure_rules, seed), region)
        merged = vae.decoder._structure_from_binary(s_bool)      # (no bar is empty: the structure stays as merged)
    s_tensor = merged.s_tensor.view(B, n_bars, 4, 32).bool()
    _, c_logits = vae.decoder(z, merged)
    tokens, _, _ = _draw(c_logits.detach().contiguous().float(), s_tensor, sampled, temperature, top_k, top_p, seed, chord_rules,
                         harmony=harmony)
    info = ops.infill_tokens(s_in, merged.s_tensor, region, graph.tokens, tokens, bar_forced)
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, s_tensor)
    out = (NoteBatch(notes, track_ptr, totals, n_bars, batch.resolution), s_tensor)
    for wanted, value in ((return_tokens, tokens), (return_z, z), (return_info, info)):
        if wanted:
            out += (value,)
    return out


@dataclass
class NoteScores:
    """What the decoder thinks of pieces (`score_graph`, `score_notes`; csrc/score.hip), device tensors for K latents of B
    pieces of n_bars bars: `content_logp` float64 [K,B,n_bars,4,2], the summed log-probabilities of the pieces' own pitch and
    duration tokens per (bar, track); `content_counts` int32 [K,B,n_bars,4,6] = nodes, pitch targets, duration targets, pitch
    hits, duration hits, note hits; `structure_logp` float64 [K,B,n_bars,4], the Bernoulli log-likelihood of the pieces' own
    cells; `structure_counts` int32 [K,B,n_bars,4,4] = cells on, predicted on, true positives, cells that agree; `row_logp`, a
    list of K float32 [N,15,2] (per node and slot); the encoder's `mu`, `log_var` [B,d] and the latents `z` [K,B,d].  The
    methods are plain torch in float64 and read nothing back."""
    content_logp: torch.Tensor
    content_counts: torch.Tensor
    structure_logp: torch.Tensor
    structure_counts: torch.Tensor
    row_logp: list
    mu: torch.Tensor
    log_var: torch.Tensor
    z: torch.Tensor

    def log_likelihood(self, structure: bool = True) -> torch.Tensor:
        """log p(x | z_k) per piece [K,B]: both heads of every token, with `structure` also the cells."""
        ll = self.content_logp.sum(dim=(2, 3, 4))
        return ll + self.structure_logp.sum(dim=(2, 3)) if structure else ll

    def per_bar(self) -> torch.Tensor:
        """The log-likelihood (tokens and cells) of every bar [K,B,n_bars]: the lowest is the bar the model finds least likely."""
        return self.content_logp.sum(dim=(3, 4)) + self.structure_logp.sum(dim=3)

    def per_track(self) -> torch.Tensor:
        """The log-likelihood (tokens and cells) of every track [K,B,4] (Drums, Bass, Guitar, Strings)."""
        return self.content_logp.sum(dim=(2, 4)) + self.structure_logp.sum(dim=2)

    def nll_per_token(self) -> torch.Tensor:
        """-log p of the tokens over their number (pitch and duration targets) [K,B]; NaN for a piece without a target."""
        n = self.content_counts[..., 1:3].sum(dim=(2, 3, 4)).double()
        return -self.content_logp.sum(dim=(2, 3, 4)) / n

    def perplexity(self) -> torch.Tensor:
        return torch.exp(self.nll_per_token())

    def accuracies(self) -> dict:
        """The reference's accuracies (training.py:438-497) per piece, each [K,B] and NaN where its denominator is 0: pitch,
        dur, note, pitch_drums (track 0), pitch_non_drums, s_precision, s_recall, s_f1."""
        c = self.content_counts.double().sum(dim=2)                # [K,B,4,6]
        s = self.structure_counts.double().sum(dim=(2, 3))         # [K,B,4]
        t = c.sum(dim=2)
        prec, rec = s[..., 2] / s[..., 1], s[..., 2] / s[..., 0]
        return {"pitch": t[..., 3] / t[..., 1], "dur": t[..., 4] / t[..., 2], "note": t[..., 5] / t[..., 1],
                "pitch_drums": c[..., 0, 3] / c[..., 0, 1],
                "pitch_non_drums": c[..., 1:, 3].sum(dim=2) / c[..., 1:, 1].sum(dim=2),
                "s_precision": prec, "s_recall": rec, "s_f1": 2 * rec * prec / (rec + prec)}

    def kl(self) -> torch.Tensor:
        """KL(q(z|x) || N(0, I)) per piece [B]: the formula of training.py:329 without its batch mean."""
        mu, lv = self.mu.double(), self.log_var.double()
        return -0.5 * (1 + lv - mu * mu - lv.exp()).sum(dim=1)

    def elbo(self, beta: float = 1.0) -> torch.Tensor:
        """log p(x | z_k) - beta KL per piece [K,B]."""
        return self.log_likelihood() - float(beta) * self.kl()

    def iwae(self) -> torch.Tensor:
        """The importance-weighted bound per piece [B]: logsumexp_k[log p(x|z_k) + log N(z_k; 0, I) - log q(z_k|x)] - log K."""
        z, mu, lv = self.z.double(), self.mu.double(), self.log_var.double()
        log_prior = -0.5 * (z * z + math.log(2 * math.pi)).sum(dim=2)
        log_q = -0.5 * ((z - mu) ** 2 / lv.exp() + lv + math.log(2 * math.pi)).sum(dim=2)
        return torch.logsumexp(self.log_likelihood() + log_prior - log_q, dim=0) - math.log(z.shape[0])


def _check_score_args(vae, graph, z, samples, seed):
    """The argument rules of `score_graph`, before anything runs."""
    tokens, s_tensor = getattr(graph, "tokens", None), getattr(graph, "s_tensor", None)
    if not isinstance(tokens, torch.Tensor) or not isinstance(s_tensor, torch.Tensor):
        raise ValueError("graph must be a BarGraphBatch with tokens and s_tensor (a DeviceLoader batch, NoteBatch.to_graph())")
    n_bars, d = vae.cfg["n_bars"], vae.cfg["d"]
    if getattr(graph, "n_bars", n_bars) != n_bars:
        raise ValueError(f"graph holds pieces of n_bars = {graph.n_bars}, the model takes n_bars = {n_bars}")
    if s_tensor.dim() != 3 or s_tensor.shape[1:] != (4, 32) or s_tensor.shape[0] == 0 or s_tensor.shape[0] % n_bars:
        raise ValueError(f"graph.s_tensor must be [B * {n_bars},4,32], got {tuple(s_tensor.shape)}")
    _check_latent_args(s_tensor.shape[0] // n_bars, d, z, samples, seed)


def _check_latent_args(B, d, z, samples, seed):
    if not (ops._integer(samples) and samples >= 1):
        raise ValueError(f"samples must be an int >= 1, got {samples!r}")
    ops.check_sampling_args(seed=seed)
    if z is not None:
        if not isinstance(z, torch.Tensor) or not z.dtype.is_floating_point or z.dim() not in (2, 3) or z.shape[-2:] != (B, d) \
                or z.shape[0] == 0:
            raise ValueError(f"z must be a float tensor [{B},{d}] or [K,{B},{d}], got "
                             f"{tuple(z.shape) if isinstance(z, torch.Tensor) else type(z).__name__}")


def _score(vae, graph, mu, log_var, z, samples, seed) -> NoteScores:
    """The core of `score_graph` and `score_notes`: one decoder pass per latent on the input's own bar graphs, each scored
    against the input's tokens and structure.  Runs inside the caller's eval / no_grad block."""
    n_bars = vae.cfg["n_bars"]
    if z is not None:
        zs = (z if z.dim() == 3 else z[None]).to(mu.device, torch.float32)
    elif samples == 1 and seed is None:
        zs = mu[None]
    else:
        gen = None if seed is None else torch.Generator().manual_seed(int(seed))
        eps = torch.randn((samples,) + tuple(mu.shape), generator=gen, dtype=torch.float32).to(mu.device)
        zs = mu[None] + torch.exp(0.5 * log_var)[None] * eps
    s_tensor = graph.s_tensor.view(-1, n_bars, 4, 32)
    out = [[], [], [], [], []]
    for zk in zs:
        s_logits, c_logits = vae.decoder(zk.contiguous(), graph)
        c_logp, c_counts, row_logp = ops.score_tokens(c_logits.detach().contiguous().float(), graph.tokens, s_tensor, check=False)
        s_logp, s_counts = ops.score_structure(s_logits.detach().reshape(s_tensor.shape).contiguous().float(), s_tensor)
        for acc, v in zip(out, (c_logp, c_counts, s_logp, s_counts, row_logp)):
            acc.append(v)
    return NoteScores(torch.stack(out[0]), torch.stack(out[1]), torch.stack(out[2]), torch.stack(out[3]), out[4], mu, log_var,
                      zs.contiguous())


def score_graph(vae, graph, z=None, samples=1, seed=None) -> NoteScores:
    """The log-likelihood of pieces under the model, per bar and track: `graph` is a `BarGraphBatch` with tokens (a
    `DeviceLoader` batch, `NoteBatch.to_graph()`).  The encoder gives (mu, log_var); every latent z_k is one
    `vae.decoder(z_k, graph)` pass on the pieces' own bar graphs, whose logits are scored against the pieces' own tokens
    (`ops.score_tokens`) and cells (`ops.score_structure`).  With `z=None, samples=1` the latent is mu; with `samples=K > 1`, or a
    `seed`, z_k = mu + exp(log_var / 2) eps_k, eps drawn on the CPU from a generator seeded with `seed` as in `vary_notes`
    (None with K > 1: torch's global generator); a `z` [B,d] or [K,B,d] overrides both.  Eval mode, no gradients,
    `vae.training` left as found; no host read.  Returns `NoteScores`."""
    _check_score_args(vae, graph, z, samples, seed)
    was_training = vae.training
    vae.eval()
    try:
        with torch.no_grad():
            mu, log_var = vae.encoder(graph)
            return _score(vae, graph, mu, log_var, z, samples, seed)
    finally:
        vae.train(was_training)


def score_notes(vae, batch, z=None, samples=1, seed=None) -> NoteScores:
    """`score_graph` for pieces held as notes (a `NoteBatch`, checked as by `encode_notes`): the bar to hand to `infill_notes`
    is `scores.per_bar().argmin(-1)`.  What is scored is what the encoder sees (`NoteBatch.to_graph`: pitches clamped to
    0..127, durations to 1..96, the first 14 notes of a cell).  No host read beyond those of `to_graph`."""
    _check_batch(vae, batch)
    _check_latent_args((batch.track_ptr.shape[0] - 1) // 4, vae.cfg["d"], z, samples, seed)
    mu, log_var, graph = _encode(vae, batch)
    was_training = vae.training
    vae.eval()
    try:
        with torch.no_grad():
            return _score(vae, graph, mu, log_var, z, samples, seed)
    finally:
        vae.train(was_training)
