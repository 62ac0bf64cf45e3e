"""Note events on the device (csrc/notes.hip, `ops.notes_from_tokens`, `generate_notes`, `NoteBatch`) against notes recorded
from the reference itself (tests/golden/<case>_notes.npz) and against the numpy restatement of its slot loop (`notes_ref`,
tests/notes_util.py, which tests/test_notes_golden.py ties to the same recording).  Integers throughout: every comparison
is exact."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import ChordRules, NoteBatch, StructureRules, generate_music, generate_notes, pitch_mask, step_mask
from polyphemus_amd.model import VAE
from notes_util import CASES, as_lists, load_case_tokens, load_notes, looped_ref, notes_ref
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
PITCHES = np.array(list(range(128)) + [128, 129, 130, -1, 131, 1 << 20, -(1 << 31)])
DURS = np.array(list(range(96)) + [96, 97, 98, -1, 99, 1 << 20, -(1 << 31)])


def synthetic(B, n_bars, p, seed, special=0.03):
    """seeded (tokens int32 [N,15,2], s bool [B,n_bars,4,32]): a cell is active with probability p; every token is a special
    one (SOS, EOS, PAD, out of range) with probability `special`, so chords of every length 0..15 occur"""
    rng = np.random.default_rng(seed)
    s = rng.random((B, n_bars, 4, 32)) < p
    N = int(s.sum())
    pw = np.r_[np.full(128, (1 - special) / 128), np.full(7, special / 7)]
    dw = np.r_[np.full(96, (1 - special) / 96), np.full(7, special / 7)]
    tokens = np.stack([rng.choice(PITCHES, (N, 15), p=pw), rng.choice(DURS, (N, 15), p=dw)], -1).astype(np.int32)
    return tokens, s


def device_notes(tokens, s, **kw):
    """(notes[:M], track_ptr, totals) as numpy, after the checks every result must pass"""
    t, sd = torch.from_numpy(np.ascontiguousarray(tokens)).to(DEV), torch.from_numpy(np.ascontiguousarray(s)).to(DEV)
    notes, track_ptr, totals = ops.notes_from_tokens(t, sd, **kw)
    N, B = tokens.shape[0], s.shape[0]
    assert notes.dtype == track_ptr.dtype == totals.dtype == torch.int32 and notes.is_cuda and track_ptr.is_cuda and totals.is_cuda
    assert notes.shape == (15 * N, 3) and track_ptr.shape == (4 * B + 1,) and totals.shape == (2,)
    ptr, tot = track_ptr.cpu().numpy(), totals.cpu().numpy()
    assert ptr[0] == 0 and ptr[-1] == tot[0] and (np.diff(ptr) >= 0).all() and tot[1] == int((np.asarray(s) != 0).sum())
    return notes[:int(tot[0])].cpu().numpy(), ptr, tot


def assert_equals_ref(tokens, s, got=None):
    notes, ptr, tot = got if got is not None else device_notes(tokens, s)
    want, want_ptr = notes_ref(tokens, s)
    assert np.array_equal(ptr, want_ptr), (ptr[:9], want_ptr[:9])
    assert notes.shape == want.shape and np.array_equal(notes, want), np.flatnonzero((notes != want).any(1))[:8]
    return notes, ptr


@pytest.mark.parametrize("name", list(CASES))
def test_golden_cases_equal_the_reference_recorded_notes(name):
    B, n_bars = CASES[name]
    _, s, c_logits = load_case_tokens(name)
    want, want_ptr = load_notes(name)
    tokens = ops.sample_tokens(torch.from_numpy(c_logits).to(DEV), 0)
    notes, track_ptr, totals = ops.notes_from_tokens(tokens, torch.from_numpy(s).to(DEV))
    N, M = c_logits.shape[0], want.shape[0]
    assert notes.dtype == torch.int32 and notes.shape == (15 * N, 3)
    assert track_ptr.dtype == torch.int32 and track_ptr.shape == (4 * B + 1,) and np.array_equal(track_ptr.cpu().numpy(), want_ptr)
    assert totals.dtype == torch.int32 and totals.cpu().tolist() == [M, N]
    assert np.array_equal(notes[:M].cpu().numpy(), want)
    for dtype in (torch.bool, torch.float32, torch.int64):        # the structure in any dtype
        again = ops.notes_from_tokens(tokens, torch.from_numpy(s).to(DEV).to(dtype))
        assert torch.equal(again[0][:M], notes[:M]) and torch.equal(again[1], track_ptr) and torch.equal(again[2], totals)


@pytest.mark.parametrize("B,n_bars,p", [(1, 1, None), (3, 3, 0.3), (3, 3, 1.0), (75, 4, 0.1), (2, 2, 0.0)],
                         ids=["one-cell", "odd-bars", "odd-bars-full", "1200-segments", "all-inactive"])
def test_synthetic_tokens_equal_the_restatement(B, n_bars, p):
    """one active cell; G = 9 bars (odd: the bar-count kernel's last half-wave has no bar); every cell active; 1200 segments,
    more than the scan's 1024 threads; no active cell at all (N = 0)"""
    if p is None:
        tokens, s = synthetic(1, 1, 1.0, 11)
        keep = 32 * 2 + 17                                        # guitar, step 17
        s = np.zeros_like(s)
        s.reshape(-1)[keep] = True
        tokens = tokens[5:6].copy()
        tokens[0, :3] = [(60, 3), (64, 40), (67, 7)]              # a chord that surely has notes
    else:
        tokens, s = synthetic(B, n_bars, p, 100 * B + n_bars)
    notes, ptr = assert_equals_ref(tokens, s)
    if p == 0.0:
        assert tokens.shape[0] == 0 and notes.shape == (0, 3) and not ptr.any()
    elif p is None:
        assert notes[:3].tolist() == [[17, 60, 4], [17, 64, 15], [17, 67, 8]] and ptr[:4].tolist() == [0, 0, 0, len(notes)]
    else:
        assert len(notes) > 15 * B


def branch_case():
    """B = 2 pieces of two bars, every branch of the slot loop by hand; piece 0 has no Bass cell and piece 1 no Guitar cell"""
    s = np.zeros((2, 2, 4, 32), bool)
    cells = [(0, 0, 0, 3), (0, 0, 2, 0), (0, 0, 3, 9), (0, 1, 0, 31), (0, 1, 3, 5),           # piece 0: nodes 0..4
             (1, 0, 0, 0), (1, 0, 1, 30), (1, 1, 1, 31), (1, 1, 3, 31)]                        # piece 1: nodes 5..8
    for c in cells:
        s[c] = True
    tok = np.full((9, 15, 2), (130, 98), np.int32)
    tok[0, :5] = [(36, 0), (128, 5), (40, 96), (41, 7), (129, 97)]   # SOS in the middle of a chord; duration token 96
    tok[1, :3] = [(60, 98), (61, 1), (129, 97)]                      # a PAD duration in front of a valid pitch
    tok[2, 0] = (129, 97)                                            # slot 0 is EOS
    tok[3, :2] = [(38, 95), (39, 0)]                                 # last step, duration token 95: clamped to 1
    tok[4, :] = [(50 + j, j) for j in range(15)]                     # 15 notes and no terminator
    tok[5, :4] = [(-1, 99), (131, -1), (5, 131), (129, 0)]           # out of range reads as 0
    tok[6, :3] = [(45, 96), (128, 97), (46, 1)]                      # token 96 clamped; an EOS duration ends on a skipped SOS too
    tok[7, :2] = [(47, 97), (48, 1)]                                 # an EOS duration in front of a valid pitch
    tok[8, :3] = [(128, 1), (128, 2), (70, 50)]                      # leading SOS pitches
    return tok, s


def test_every_branch_of_the_slot_loop():
    tok, s = branch_case()
    got = device_notes(tok, s)
    notes, ptr = assert_equals_ref(tok, s, got)
    assert ptr.tolist() == [0, 5, 5, 5, 20, 23, 24, 24, 25]          # empty tracks: equal entries, still in order
    assert notes[:5].tolist() == [[3, 36, 1], [3, 40, 61], [3, 41, 8], [63, 38, 1], [63, 39, 1]]
    assert notes[5:20].tolist() == [[37, 50 + j, j + 1] for j in range(15)]
    assert notes[20:23].tolist() == [[0, 0, 1], [0, 0, 1], [0, 5, 1]]
    assert notes[23:].tolist() == [[30, 45, 34], [63, 70, 1]]
    pieces = as_lists(notes, ptr)
    assert pieces[0][1] == [] and pieces[0][2] == [] and pieces[1][1] == [(30, 45, 34)] and pieces[1][2] == [] and pieces[1][3] == [(63, 70, 1)]


def test_notes_equal_the_pianoroll_path_on_the_same_tokens():
    """`notes_ref` on the per-head arg-max of `ops.mtp_from_tokens(tokens, s)`, which is what the reference would read"""
    for tokens, s in (synthetic(3, 3, 0.3, 21, special=0.08), branch_case()):
        t, sd = torch.from_numpy(tokens).to(DEV), torch.from_numpy(s).to(DEV)
        mtp = ops.mtp_from_tokens(t, sd)
        cells = mtp.reshape(-1, 15, 230)[sd.reshape(-1)]
        read = torch.stack([cells[..., :131].argmax(-1), cells[..., 131:].argmax(-1)], -1).cpu().numpy()
        assert (read != tokens).any()                             # out-of-range tokens came back as 0
        want, want_ptr = notes_ref(read, s)
        notes, ptr, _ = device_notes(tokens, s)
        assert np.array_equal(ptr, want_ptr) and np.array_equal(notes, want)


def _raw(tokens, s, N, rows, sentinel, pad=6):
    """pm_notes_from_tokens through the raw binding on a notes buffer of `rows` rows pre-filled with a sentinel, `pad` ints of
    it on either side: (whole buffer, track_ptr, totals) as numpy"""
    B, n_bars = s.shape[:2]
    G = B * n_bars
    t = torch.from_numpy(tokens).to(DEV)
    sf = torch.from_numpy(s).to(DEV).float().contiguous()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=DEV)
    seg_count, seg_ptr, bn, npt, track_ptr, totals = i32(4 * G), i32(4 * G + 1), i32(G), i32(G + 1), i32(4 * B + 1), i32(2)
    buf = torch.full((pad + 3 * rows + pad,), sentinel, dtype=torch.int32, device=DEV)
    _lib.call("pm_notes_from_tokens", t.data_ptr(), sf.data_ptr(), G, n_bars, N, seg_count.data_ptr(), seg_ptr.data_ptr(),
              bn.data_ptr(), npt.data_ptr(), buf.data_ptr() + 4 * pad, rows, track_ptr.data_ptr(), totals.data_ptr(), _lib.stream())
    return buf.cpu().numpy(), track_ptr.cpu().numpy(), totals.cpu().numpy()


def test_rows_from_m_on_are_untouched_and_two_calls_write_the_same_bytes():
    sentinel, pad = -123456789, 6
    tokens, s = synthetic(5, 2, 0.25, 31)
    N = tokens.shape[0]
    want, want_ptr = notes_ref(tokens, s)
    M = len(want)
    assert 0 < M < 15 * N
    for rows in (15 * N, 15 * N + 9):
        buf, ptr, tot = _raw(tokens, s, N, rows, sentinel, pad)
        assert tot.tolist() == [M, N] and np.array_equal(ptr, want_ptr)
        assert np.array_equal(buf[pad:pad + 3 * M].reshape(M, 3), want)
        assert (buf[:pad] == sentinel).all() and (buf[pad + 3 * M:] == sentinel).all()
        again = _raw(tokens, s, N, rows, sentinel, pad)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((buf, ptr, tot), again))
    # fewer nodes than active cells: the cells beyond N are silent, nothing else moves
    buf, ptr, tot = _raw(tokens[:N - 4].copy(), s, N - 4, 15 * (N - 4), sentinel, pad)
    want4, want4_ptr = notes_ref(tokens[:N - 4], s)
    assert tot.tolist() == [len(want4), N] and np.array_equal(ptr, want4_ptr)
    assert np.array_equal(buf[pad:pad + 3 * len(want4)].reshape(-1, 3), want4) and (buf[pad + 3 * len(want4):] == sentinel).all()


def test_check_raises_on_a_node_count_that_differs_from_the_active_cells():
    tokens, s = synthetic(2, 2, 0.2, 41)
    N = tokens.shape[0]
    t, sd = torch.from_numpy(tokens).to(DEV), torch.from_numpy(s).to(DEV)
    ops.notes_from_tokens(t, sd)
    more = torch.cat([t, t[:1]])
    for bad in (t[:-1].contiguous(), more):
        with pytest.raises(ValueError, match="shape mismatch"):
            ops.notes_from_tokens(bad, sd)
        with pytest.raises(ValueError, match="shape mismatch"):
            ops.notes_from_tokens(bad, sd, check=True)
    notes, ptr, tot = ops.notes_from_tokens(t[:-1].contiguous(), sd, check=False)          # the caller's risk, as mtp_from_tokens
    want, want_ptr = notes_ref(tokens[:-1], s)
    assert tot.cpu().tolist() == [len(want), N] and np.array_equal(ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(notes[:len(want)].cpu().numpy(), want)
    notes, ptr, tot = ops.notes_from_tokens(more, sd, check=False)                          # a node no cell refers to
    want, want_ptr = notes_ref(tokens, s)
    assert tot.cpu().tolist() == [len(want), N] and np.array_equal(notes[:len(want)].cpu().numpy(), want)
    with pytest.raises(ValueError, match="tokens"):
        ops.notes_from_tokens(t.long(), sd)
    with pytest.raises(ValueError, match="s_tensor"):
        ops.notes_from_tokens(t, sd[0])
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.notes_from_tokens(t, sd.cpu())


# ---- end to end -----------------------------------------------------------------------------------------------------------
E2E_CHORDS = ChordRules(min_notes=(1, 1, 2, 0), max_notes=(14, 1, 6, 14),
                        allowed_pitches=np.stack([pitch_mask(), pitch_mask(28, 60), pitch_mask(40, 88, (0, 2, 4, 5, 7, 9, 11)),
                                                  pitch_mask(60, 62)]))
E2E_STRUCTURE = StructureRules(temperature=1.0, threshold=(0.5, 0.4, 0.5, 0.6), min_active=(1, 0, 0, 0), max_active=(16, 8, 12, 4),
                               allowed_steps=np.stack([step_mask(), step_mask(2), step_mask(), step_mask(4)]))
MODES = {"unsampled": dict(), "sampled": dict(temperature=0.8, seed=7), "chords": dict(chord_rules=E2E_CHORDS, seed=7),
         "structure+chords": dict(structure_rules=E2E_STRUCTURE, chord_rules=E2E_CHORDS, seed=7)}


class _Record:
    def __init__(self, *a, **kw):
        self.args = a
        self.__dict__.update(kw)


def fake_muspy():
    m = types.ModuleType("muspy")
    for name in ("Note", "Track", "Metadata", "Music"):
        setattr(m, name, type(name, (_Record,), {}))
    return m


def cell_counts(pieces, s):
    """notes per active cell, in node (cell) order, from the lists of `tolist()`"""
    s = np.asarray(s) != 0
    out = []
    for i, b, k, step in np.argwhere(s):
        out.append(sum(1 for (t, _, _) in pieces[i][k] if t == 32 * b + step))
    return np.asarray(out)


@pytest.mark.parametrize("name", list(CASES))
def test_generate_notes_end_to_end(name, monkeypatch):
    z, cfg = load_case(name)
    gg = np.load(os.path.join(GOLDEN, f"{name}_generate.npz"), allow_pickle=False)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    zs = torch.from_numpy(gg["gen/z"]).to(DEV)
    n_bars = cfg["n_bars"]
    programs = {"Drums": -1, "Bass": 34, "Guitar": 1, "Strings": 83}
    with torch.no_grad():
        for mode, kw in MODES.items():
            chords = "chord_rules" in kw
            ref = generate_music(vae, zs, return_tokens=True, return_note_counts=chords, **kw)
            out = generate_notes(vae, zs, return_tokens=True, **kw)
            assert len(out) == 3 and isinstance(out[0], NoteBatch), mode
            batch, s_tensor, tokens = out
            assert torch.equal(s_tensor, ref[1]) and torch.equal(tokens, ref[2]) and tokens.dtype == torch.int32, mode
            assert batch.n_bars == n_bars and batch.resolution == 8 and batch.notes.is_cuda
            short = generate_notes(vae, zs, **kw)
            assert len(short) == 2 and torch.equal(short[0].track_ptr, batch.track_ptr) and torch.equal(short[1], s_tensor), mode
            M = int(batch.totals[0])
            assert torch.equal(short[0].notes[:M], batch.notes[:M]) and torch.equal(short[0].totals, batch.totals), mode
            want, want_ptr = notes_ref(tokens.cpu().numpy(), s_tensor.cpu().numpy())
            pieces = batch.tolist()
            assert pieces == as_lists(want, want_ptr) and len(pieces) == zs.shape[0] and M == len(want) > 0, mode
            assert all(type(v) is int for v in pieces[0][0][0]) if pieces[0][0] else True
            if chords:
                assert np.array_equal(cell_counts(pieces, s_tensor.cpu().numpy()), ref[3].cpu().numpy()), mode
            assert batch.looped(3) == looped_ref(pieces, 3, n_bars) and batch.looped(1) == pieces, mode
            assert sum(len(t) for p in batch.looped(3) for t in p) == 3 * M
        # the drawn structure differs from the thresholded one, and the rules hold on it
        assert not torch.equal(s_tensor, generate_notes(vae, zs)[1])
        assert int(s_tensor[:, :, 3].sum(-1).max()) <= 4 and not bool(s_tensor[:, :, 1, 1::2].any())
        # to_muspy against a stand-in module
        monkeypatch.setitem(sys.modules, "muspy", fake_muspy())
        i = zs.shape[0] - 1
        music = batch.to_muspy(i, programs)
        assert type(music).__name__ == "Music" and music.resolution == 8 and type(music.metadata).__name__ == "Metadata"
        assert [t.name for t in music.tracks] == ["Drums", "Bass", "Guitar", "Strings"]
        assert [t.is_drum for t in music.tracks] == [True, False, False, False] and [t.program for t in music.tracks] == [0, 34, 1, 83]
        assert [[n.args for n in t.notes] for t in music.tracks] == [[(t_, p, d, 64) for (t_, p, d) in tr] for tr in pieces[i]]
        # never the pianoroll
        def boom(*a, **k):
            raise AssertionError("generate_notes must not build the pianoroll")
        monkeypatch.setattr(ops, "mtp_from_tokens", boom)
        monkeypatch.setattr(ops, "mtp_from_logits", boom)
        for mode, kw in MODES.items():
            again = generate_notes(vae, zs, **kw)[0]
            if mode == "structure+chords":
                assert again.tolist() == pieces
        with pytest.raises(AssertionError, match="pianoroll"):
            generate_music(vae, zs)
