"""Host mirror of the reference's generation entry points (generate.py:21-37, 90-98) over the device kernels of
csrc/generate.hip and csrc/graph.hip: the decoder pass, the thresholded structure, and the dense multitrack pianoroll,
without the reference's host synchronisations (`nonzero`, per-sample Python graph building, three full-tensor writes).
Converting the pianoroll to MIDI (muspy) is outside the hot path and stays with the caller; `generate_notes` returns the
pieces as ordered note events instead (`NoteBatch`, csrc/notes.hip), which is what that conversion reads out of the pianoroll.
The other direction has no entry point in the reference: `NoteBatch.from_lists` / `to_graph` (csrc/notes_in.hip) turn notes into the
batch the encoder consumes, `encode_notes` and `vary_notes` encode a piece and decode around it."""
from __future__ import annotations

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


def _decode(vae, z, s_cond, s_tensor_cond, rules=None, seed=None):
    """the decoder pass of `generate_music`: (c_logits [N,15,230] fp32, s_tensor).  With `rules` (a StructureRules) the
    structure is drawn from the structure logits on the device under `seed` and the content decoder runs on its bar graphs."""
    vae.decoder.__dict__.pop("_last_structure", None)
    if rules is not None:
        with torch.no_grad():
            s_logits = vae.engine.structure_only(z.contiguous().float(), vae.training)
        s_tensor = ops.sample_structure(s_logits.detach().contiguous().float(), rules.temperature, rules.threshold,
                                        rules.min_active, rules.max_active, rules.allowed_steps, seed)
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
                   return_tokens=False, chord_rules=None, return_note_counts=False, structure_rules=None):
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
    with different rhythms.  No host read is added to the one that sizes the bar graphs."""
    tokens, s_tensor, note_count, c_logits = _decode_and_draw(vae, z, s_cond, s_tensor_cond, temperature, top_k, top_p, seed,
                                                              chord_rules, structure_rules, return_note_counts, return_tokens)
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
                     return_note_counts=False, argmax_tokens=True):
    """The part `generate_music` and `generate_notes` share: the argument checks, the seed, the decoder pass and the draw.
    Returns (tokens int32 [N,15,2], s_tensor, note_count int32 [N] or None without chord rules, c_logits): c_logits is None
    in every sampled mode; in the unsampled one it holds the content logits and `tokens` their arg-max (None when
    `argmax_tokens` is off: the caller lays the logits out and wants no tokens)."""
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
        sampled = True
    else:
        if return_note_counts:
            raise ValueError("return_note_counts needs chord_rules")
        ops.check_sampling_args(temperature, top_k, top_p, seed)
        sampled = temperature is not None or top_k is not None or top_p is not None
    if structure_rules is not None and seed is None:             # one seed for both levels, drawn before the structure
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())
    c_logits, s_tensor = _decode(vae, z, s_cond, s_tensor_cond, structure_rules, seed)
    if not sampled:
        return (ops.sample_tokens(c_logits, temperature=0.0) if argmax_tokens else None), s_tensor, None, c_logits
    if seed is None:
        seed = int(torch.randint(0, 1 << 32, (1,), dtype=torch.int64).item())
    if chord_rules is None:
        tokens = ops.sample_tokens(c_logits, 1.0 if temperature is None else temperature, top_k, top_p, seed)
        return tokens, s_tensor, None, None
    track = ops.node_tracks(s_tensor, c_logits.shape[0], check=False)
    tokens, note_count = ops.sample_chords(c_logits, track, 1.0 if temperature is None else temperature, top_k, top_p, seed,
                                           chord_rules.min_notes, chord_rules.max_notes, chord_rules.allowed_pitches)
    return tokens, s_tensor, note_count, None


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


def generate_notes(vae, z, s_cond=None, s_tensor_cond=None, *, temperature=None, top_k=None, top_p=None, seed=None,
                   chord_rules=None, structure_rules=None, return_tokens=False):
    """`generate_music` without the pianoroll: the same arguments, checks, seed handling and draws in every mode (unsampled =
    the arg-max tokens), but the pieces come back as a `NoteBatch` — the notes the reference's `muspy_from_mtp` would read out
    of `generate_music`'s `mtp`, in its order — read from the tokens on the device (`ops.notes_from_tokens`).  Returns
    (NoteBatch, s_tensor), with `return_tokens` the int32 [N,15,2] tokens appended.  One host read beyond the one that sizes
    the bar graphs: the check that the structure has as many active cells as the decoder gave nodes."""
    tokens, s_tensor, _, _ = _decode_and_draw(vae, z, s_cond, s_tensor_cond, temperature, top_k, top_p, seed, chord_rules,
                                              structure_rules)
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, s_tensor)
    batch = NoteBatch(notes, track_ptr, totals, int(s_tensor.shape[1]))
    return (batch, s_tensor, tokens) if return_tokens else (batch, s_tensor)


def _encode(vae, batch):
    """(mu, log_var, graph) of a NoteBatch: the encoder in eval mode without gradients, the mode it found restored."""
    if not isinstance(batch, NoteBatch):
        raise ValueError(f"batch must be a NoteBatch, got {type(batch).__name__}")
    if batch.n_bars != vae.cfg["n_bars"]:
        raise ValueError(f"batch holds pieces of n_bars = {batch.n_bars}, the model takes n_bars = {vae.cfg['n_bars']}")
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
    Every other keyword is `generate_notes`'.  Returns what `generate_notes` returns, (NoteBatch, s_tensor[, tokens]), with
    `return_z` the latent appended."""
    if not (ops._real(strength) and np.isfinite(strength) and strength >= 0):
        raise ValueError(f"strength must be a finite number >= 0, got {strength!r}")
    ops.check_sampling_args(seed=seed)
    for k in ("s_cond", "s_tensor_cond"):
        if k in generate_notes_kwargs:
            raise ValueError(f"{k} is not an argument of vary_notes: keep_structure=True passes the input's structure")
    if keep_structure and generate_notes_kwargs.get("structure_rules") is not None:
        raise ValueError("structure_rules draws the structure itself: it needs s_cond and s_tensor_cond both None")
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
