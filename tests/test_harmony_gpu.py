"""Harmony on the device ("Harmony" in include/polyphemus_hip.h): pm_sample_chords_at (k_sample_chords<MODE, true> of
csrc/sample.hip) against the fp64 replica of tests/test_chords_gpu.py run with per-node rules, bit-identity with
pm_sample_chords where the chart cannot bind, the invariants of a chart, pm_node_cells (csrc/generate.hip) against numpy,
pm_note_chroma (csrc/stats.hip) against the numpy restatement of tests/harmony_util.py and against pm_note_stats,
`NoteBatch.harmony` on a hand-made batch, and `harmony=` end to end on the golden tiny models."""
import ctypes
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import (TRACKS, ChordRules, Harmony, NoteBatch, StructureRules, generate_music, generate_notes,
                                     infill_notes, pick_takes, region_mask, vary_song)
from polyphemus_amd.model import VAE
from harmony_util import A_MINOR, C_MAJOR, FREE, SETS, chroma_ref, random_rows, sets_ref
from test_chords_gpu import (ALLOWED, CONFIGS, EOS_D, EOS_P, LEFT_OUT_CAP, MAX_NOTES, MIN_NOTES, PAD_D, PAD_P, SCALES, make_logits,
                             replica, tracks_of)
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 5, 273)
BOUND = 0b1110                                                   # the chart binds Bass, Guitar and Strings
SENTINEL = -123456789


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layout(N):
    """(track [N], set [N], node_cell int32 [N], chart int32 [G,32]): node n is the cell (bar n // 32, track, step n % 32) and
    that cell of the chart carries set[n] = SETS[(5 n + n // 7) % 6]; the cells without a node are free"""
    n = np.arange(N)
    track = tracks_of(N)
    sets = np.array([SETS[(5 * i + i // 7) % 6] for i in n], np.int64)
    cell = (128 * (n // 32) + 32 * track + n % 32).astype(np.int32)
    chart = np.full(((N + 31) // 32, 32), FREE, np.int32)
    chart[n // 32, n % 32] = sets
    return track, sets, cell, chart


def class_mask(sets):
    """[N,128] bool: pitch p has its class in set n"""
    return ((np.asarray(sets)[:, None] >> (np.arange(128) % 12)[None, :]) & 1).astype(bool)


def node_rules(N):
    """the per-node rules the replica takes with track = arange(N): (min_notes [N], max_notes [N], allowed [N,128])"""
    track, sets, _, _ = layout(N)
    allowed = ALLOWED[track] & np.where((track >= 1)[:, None], class_mask(sets), True)
    return np.asarray(MIN_NOTES)[track], np.asarray(MAX_NOTES)[track], allowed


_CASES = {}


def case(N, scale, i):
    """(device tokens, device counts, replica tokens, replica counts, decided) of one case, computed once"""
    key = (N, scale, i)
    if key not in _CASES:
        Tp, Td, k, p = CONFIGS[i]
        logits = make_logits(N, scale)
        _, _, cell, chart = layout(N)
        tok, cnt = ops.sample_chords_at(logits.to(DEV), dev(cell), dev(chart), BOUND, (Tp, Td), k, p, 1000 + i, MIN_NOTES, MAX_NOTES, ALLOWED)
        assert tok.shape == (N, 15, 2) and tok.dtype == torch.int32 and cnt.shape == (N,) and cnt.dtype == torch.int32
        mn, mx, allowed = node_rules(N)
        want = replica(logits.numpy(), np.arange(N), Tp, Td, k, p, 1000 + i, mn, mx, allowed)
        _CASES[key] = (tok.cpu().numpy(), cnt.cpu().numpy()) + want
    return _CASES[key]


# ---- 1. the replica ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_chords_under_a_chart_equal_the_fp64_replica(N):
    """The replica of tests/test_chords_gpu.py with a rule per node (track = arange(N)).  At exactly these inputs the replica
    alone leaves out no node at N = 1 and N = 5 and at most 0.0256 of the nodes at N = 273; the cap is 0.05.  At N = 273,
    scale 1, configuration 0 it has 30 nodes without a pitch candidate and chords of every length 0..14."""
    hist = np.zeros(15, np.int64)
    for scale in SCALES:
        for i in range(len(CONFIGS)):
            got, got_n, want, want_n, decided = case(N, scale, i)
            left_out = 1.0 - decided.mean()
            differ = int(((got != want).any((1, 2)) | (got_n != want_n))[decided].sum())
            print(f"N={N} scale={scale} config={CONFIGS[i]}: {left_out:.4f} of the nodes left out, {differ} decided nodes differ")
            assert left_out <= LEFT_OUT_CAP, (N, scale, i, left_out)
            assert np.array_equal(got[decided], want[decided]), (N, scale, i, np.flatnonzero((got != want).any((1, 2)) & decided)[:8])
            assert np.array_equal(got_n[decided], want_n[decided]), (N, scale, i)
            hist += np.bincount(want_n, minlength=15)
    if N == 273:
        _, _, want, want_n, _ = case(273, 1, 0)
        none = ~node_rules(273)[2].any(1)
        one = np.bincount(want_n, minlength=15)
        print("note counts of the replica at scale 1, configuration 0:", one.tolist(), "over the eight cases:", hist.tolist())
        assert none.sum() == 30 and (want_n[none] == 0).all() and (want[none, 0] == (EOS_P, EOS_D)).all()
        assert (one > 0).all() and (hist > 0).all(), (one, hist)     # the test keeps exercising chords of every length 0..14


# ---- 2. bit-identity with the existing sampler ------------------------------------------------------------------------------
SAME_AS = [(Tp, Td, k, p, 1000 + i) for i, (Tp, Td, k, p) in enumerate(CONFIGS)] + [(0.0, 0.0, None, None, 3), (0.0, 1.0, 7, None, 4)]


@pytest.mark.parametrize("Tp,Td,k,p,seed", SAME_AS)
def test_a_chart_that_cannot_bind_gives_the_tokens_of_sample_chords(Tp, Td, k, p, seed):
    for N in (5, 273):
        track, _, cell, chart = layout(N)
        x = make_logits(N, 1).to(DEV)
        rules = dict(min_notes=MIN_NOTES, max_notes=MAX_NOTES, allowed_pitches=ALLOWED)
        want, want_n = ops.sample_chords(x, dev(track.astype(np.uint8)), (Tp, Td), k, p, seed, **rules)
        free = ops.sample_chords_at(x, dev(cell), dev(np.full_like(chart, FREE)), 0b1111, (Tp, Td), k, p, seed, **rules)
        unbound = ops.sample_chords_at(x, dev(cell), dev(chart), 0, (Tp, Td), k, p, seed, **rules)
        for tok, cnt in (free, unbound):
            assert torch.equal(tok, want) and torch.equal(cnt, want_n), (N, Tp, Td, k, p)
        bound = ops.sample_chords_at(x, dev(cell), dev(chart), BOUND, (Tp, Td), k, p, seed, **rules)
        assert N < 273 or not torch.equal(bound[0], want)                       # the chart of `layout` does bind


# ---- 3. invariants ----------------------------------------------------------------------------------------------------------
def test_invariants_of_a_chart():
    N, seed = 273, 31
    track, sets, cell, chart = layout(N)
    x = make_logits(N, 1).to(DEV)
    rules = dict(min_notes=1, max_notes=MAX_NOTES, allowed_pitches=ALLOWED)
    tok_d, cnt_d = ops.sample_chords_at(x, dev(cell), dev(chart), BOUND, 1.0, None, None, seed, **rules)
    tok, cnt = tok_d.cpu().numpy(), cnt_d.cpu().numpy()
    inside = class_mask(sets)
    notes = 0
    for n in range(N):
        c, t = int(cnt[n]), int(track[n])
        p = tok[n, :c, 0]
        assert (p < 128).all() and len(set(p.tolist())) == c and ALLOWED[t][p].all() and c <= MAX_NOTES[t], (n, tok[n])
        assert tuple(tok[n, c]) == (EOS_P, EOS_D) and (tok[n, c + 1:] == (PAD_P, PAD_D)).all(), (n, tok[n])
        if t >= 1:
            assert inside[n][p].all(), (n, hex(int(sets[n])), p)                # every drawn pitch has its class in the set
            notes += c
            if sets[n] == 0:
                assert c == 0 and tuple(tok[n, 0]) == (EOS_P, EOS_D)            # an empty chord, also under min_notes = 1
            elif (ALLOWED[t] & inside[n]).any():
                assert c >= 1
    assert notes > 200 and ((sets == 0) & (track >= 1)).sum() == 30
    # the drums' draws are those of the sampler without a chart
    plain, plain_n = ops.sample_chords(x, dev(track.astype(np.uint8)), 1.0, None, None, seed, **rules)
    drums = dev(track == 0)
    assert torch.equal(tok_d[drums], plain[drums]) and torch.equal(cnt_d[drums], plain_n[drums]) and int(drums.sum()) > 60
    assert not torch.equal(tok_d, plain)
    # bits 12..31 of the chart are ignored
    high = np.random.default_rng(5).integers(0, 1 << 20, chart.shape).astype(np.int64) << 12
    noisy = ((chart.astype(np.int64) | high) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    assert (noisy != chart).mean() > 0.9 and (noisy < 0).any()
    tok2, cnt2 = ops.sample_chords_at(x, dev(cell), dev(noisy), BOUND, 1.0, None, None, seed, **rules)
    assert torch.equal(tok2, tok_d) and torch.equal(cnt2, cnt_d)
    # a guard band around tokens, note_count and chart stays as it was, whatever the cells say
    pad = 37
    r = _lib.PmChordRules()
    r.temperature[0] = r.temperature[1] = 1.0
    r.top_k, r.top_p = 0, 1.0
    mask = ops.check_chord_args(allowed_pitches=ALLOWED)[3]
    for k in range(4):
        r.min_notes[k], r.max_notes[k] = 1, MAX_NOTES[k]
        for w in range(4):
            r.pitch_mask[k][w] = mask[k][w]
    G = chart.shape[0]
    wild = cell.copy()
    wild[::5] = 128 * G + 32 * track[::5] + 7                                   # a bar behind the chart: clamped to its last word
    wild[1::5] = -128 * 3 + 32 * track[1::5]                                    # a bar in front of it: clamped to its first
    for cells in (cell, wild):
        tbuf = torch.full((pad + N * 30 + pad,), SENTINEL, dtype=torch.int32, device=DEV)
        cbuf = torch.full((pad + N + pad,), SENTINEL, dtype=torch.int32, device=DEV)
        hbuf = torch.full((pad + G * 32 + pad,), 0x0AAA, dtype=torch.int32, device=DEV)
        hbuf[pad:pad + G * 32] = dev(chart).flatten()
        before = hbuf.clone()
        _lib.call("pm_sample_chords_at", x.data_ptr(), dev(cells).data_ptr(), N, hbuf.data_ptr() + 4 * pad, G, BOUND, ctypes.addressof(r),
                  seed, tbuf.data_ptr() + 4 * pad, cbuf.data_ptr() + 4 * pad, _lib.stream())
        out, cout = tbuf.cpu().numpy(), cbuf.cpu().numpy()
        assert (out[:pad] == SENTINEL).all() and (out[-pad:] == SENTINEL).all() and (cout[:pad] == SENTINEL).all() and (cout[-pad:] == SENTINEL).all()
        assert torch.equal(hbuf, before)
        t2 = out[pad:-pad].reshape(N, 15, 2)
        assert t2.min() >= 0 and (t2[..., 0] < 131).all() and (t2[..., 1] < 99).all() and cout[pad:-pad].min() >= 0 and cout[pad:-pad].max() <= 14
        if cells is cell:
            assert np.array_equal(t2, tok) and np.array_equal(cout[pad:-pad], cnt)
        else:                                                                     # the clamped cells read words of the chart itself
            at = np.clip((wild >> 7) * 32 + (wild & 31), 0, 32 * G - 1)
            seen = class_mask(chart.flatten()[at])
            for n in np.flatnonzero(track >= 1):
                assert seen[n][t2[n, :cout[pad + n], 0]].all(), n
        tbuf2 = torch.full((pad + N * 30 + pad,), SENTINEL, dtype=torch.int32, device=DEV)       # note_count may be NULL
        _lib.call("pm_sample_chords_at", x.data_ptr(), dev(cells).data_ptr(), N, hbuf.data_ptr() + 4 * pad, G, BOUND, ctypes.addressof(r),
                  seed, tbuf2.data_ptr() + 4 * pad, None, _lib.stream())
        assert torch.equal(tbuf2, tbuf)
    tok0, cnt0 = ops.sample_chords_at(x[:0].contiguous(), dev(cell[:0]), dev(chart))
    assert tok0.shape == (0, 15, 2) and cnt0.shape == (0,)


# ---- 4. the cells of the nodes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,p", [(1, 1.0), (5, 0.3), (64, 0.02), (33, 0.97), (1, 0.0)])
def test_node_cells_are_the_cell_indices_in_cell_order(G, p):
    s = torch.rand(1, G, 4, 32, generator=torch.Generator().manual_seed(G)) < p
    want = np.flatnonzero(s.numpy().reshape(-1)).astype(np.int32)                # 128 g + 32 track + step, ascending
    N = int(s.sum())
    got = ops.node_cells(s.to(DEV), N)
    assert got.dtype == torch.int32 and got.shape == (N,) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.node_cells(s.float().to(DEV), N).cpu().numpy(), want)
    assert torch.equal(((got >> 5) & 3).to(torch.uint8), ops.node_tracks(s.to(DEV), N))
    with pytest.raises(ValueError, match="active cells"):
        ops.node_cells(s.to(DEV), N + 1)
    if N:
        with pytest.raises(ValueError, match="active cells"):
            ops.node_cells(s.to(DEV), N - 1)


def test_node_cells_zero_the_tail_and_write_nothing_behind_it():
    G, pad = 5, 7
    s = (torch.rand(1, G, 4, 32, generator=torch.Generator().manual_seed(G)) < 0.3)
    want = np.flatnonzero(s.numpy().reshape(-1)).astype(np.int32)
    active = int(s.sum())
    sf = s.float().contiguous().to(DEV)
    for N in (active + 9, active, active - 4):
        buf = torch.full((pad + N + pad,), SENTINEL, dtype=torch.int32, device=DEV)
        bn, npt = torch.empty(G, dtype=torch.int32, device=DEV), torch.empty(G + 1, dtype=torch.int32, device=DEV)
        _lib.call("pm_node_cells", sf.data_ptr(), G, N, bn.data_ptr(), npt.data_ptr(), buf.data_ptr() + 4 * pad, _lib.stream())
        out = buf.cpu().numpy()
        assert (out[:pad] == SENTINEL).all() and (out[-pad:] == SENTINEL).all(), N
        assert np.array_equal(out[pad:pad + min(N, active)], want[:N]) and (out[pad + active:pad + N] == 0).all(), N
        assert int(npt[G]) == active and torch.equal(bn.cpu().long(), s.reshape(G, -1).sum(1))
    got = ops.node_cells(s.to(DEV), active + 9, check=False).cpu().numpy()
    assert np.array_equal(got[:active], want) and (got[active:] == 0).all()
    assert ops.node_cells(s.to(DEV)[:, :0], 0).shape == (0,)


# ---- 5. the chromagram ------------------------------------------------------------------------------------------------------
def chroma_batch(B, n_bars, seed):
    """(notes [M,3], track_ptr [4B+1]) of random rows (harmony_util.random_rows) with an empty track, a track of one row, one of
    more than 256 rows (the threads' stride), notes across every chunk line of a 64-bar piece and across the piece's end, rows
    behind the last track, and a track_ptr that starts below 0, steps back once and ends beyond M"""
    L = 32 * n_bars
    rng = np.random.default_rng(seed)
    sizes = [int(rng.integers(0, 50)) for _ in range(4 * B)]
    sizes[0], sizes[1], sizes[2] = 0, 1, 300
    rows = [random_rows(rng, n, L) for n in sizes]
    edges = [(x - 1, 60 + j, 96) for j, x in enumerate((512, 1024, 1536, L)) if x <= L] + [(L - 3, 7, 2), (L - 3, 8, 3), (L - 3, 9, 4), (0, 127, 1)]
    rows[3] = np.concatenate([rows[3], np.asarray(edges, np.int32)])
    sizes[3] = len(rows[3])
    notes = np.concatenate(rows + [random_rows(rng, 9, L)])                      # nine rows that belong to no track
    ptr = np.cumsum([0] + sizes).astype(np.int32)
    ptr[0] = -3
    if B > 1:
        ptr[6] = ptr[5] - 2                                                       # a step back: track 5 is empty, track 6 longer
    ptr[-1] = len(notes) + 50
    return notes, ptr


CHROMA_SHAPES = [(B, n_bars, seg) for (B, n_bars) in ((1, 1), (5, 3), (2, 64)) for seg in (1, 8, 32)] + [(3, 17, 4), (1, 16, 2), (2, 33, 16)]


@pytest.mark.parametrize("B,n_bars,seg_steps", CHROMA_SHAPES)
def test_chroma_equals_the_restatement_bit_for_bit(B, n_bars, seg_steps):
    notes, ptr = chroma_batch(B, n_bars, seed=100 * n_bars + B)
    want = chroma_ref(notes, ptr, n_bars, seg_steps)
    S = 32 * n_bars // seg_steps
    pad = 64
    nd, pd = dev(notes), dev(ptr)
    outs = []
    for fill in (SENTINEL, 0x5A5A5A5A):                                          # every word is written on every call
        buf = torch.full((4 * B * S * 12 + pad,), fill, dtype=torch.int32, device=DEV)
        _lib.call("pm_note_chroma", nd.data_ptr(), pd.data_ptr(), B, len(notes), n_bars, seg_steps, buf.data_ptr(), _lib.stream())
        a = buf.cpu().numpy()
        assert (a[-pad:] == fill).all()
        outs.append(a[:-pad].reshape(4 * B, S, 12))
    assert np.array_equal(outs[0], want), np.argwhere(outs[0] != want)[:8].tolist()
    assert np.array_equal(outs[1], outs[0])                                      # bit-identical between two calls
    wrapped = ops.note_chroma(nd, pd, n_bars, seg_steps)
    assert wrapped.dtype == torch.int32 and wrapped.shape == (4 * B, S, 12) and np.array_equal(wrapped.cpu().numpy(), want)
    assert want.sum() > 0 and (want.reshape(4 * B, -1).sum(1) == 0).any()
    # the existing kernel counts the same (note, step) pairs
    batch = NoteBatch(nd, pd, torch.zeros(2, dtype=torch.int32, device=DEV), n_bars)
    chroma = batch.chroma(seg_steps)
    assert chroma.shape == (B, 4, S, 12) and torch.equal(chroma.sum((-1, -2)).to(torch.int32), batch.stats().field("note_steps"))
    # the order of a track's rows does not matter
    shuffled = notes.copy()                                                      # (track 2 holds the rows 1 .. 300)
    shuffled[1:301] = shuffled[1:301][np.random.default_rng(1).permutation(300)]
    assert np.array_equal(ops.note_chroma(dev(shuffled), pd, n_bars, seg_steps).cpu().numpy(), want)


def test_chroma_of_no_rows():
    ptr = torch.zeros(9, dtype=torch.int32, device=DEV)
    c = ops.note_chroma(torch.zeros(0, 3, dtype=torch.int32, device=DEV), ptr, 3, 8)
    assert c.shape == (8, 12, 12) and not c.any()


# ---- 6. the harmony of a batch ----------------------------------------------------------------------------------------------
def hand_made_batch():
    """two pieces of three bars.  Piece 0: a C-major bar, an A-minor bar with a passing D in the guitar, a bar in which only
    the drums play.  Piece 1: silence, then G and B alone (G major before E minor), then a bar that changes chord half way."""
    p0 = [[(0, 36, 2), (64, 38, 2), (70, 42, 1)],
          [(0, 36, 32), (32, 45, 30)],
          [(0, 64, 8), (8, 67, 8), (16, 72, 16), (32, 60, 16), (48, 62, 2), (50, 64, 14)],
          [(0, 48, 32), (0, 52, 32), (0, 55, 32), (32, 57, 32), (32, 60, 32), (32, 64, 32)]]
    p1 = [[], [(40, 43, 8)], [(48, 59, 4)], [(64, 48, 16), (64, 52, 16), (80, 53, 16), (80, 57, 16), (80, 60, 16)]]
    return NoteBatch.from_lists([p0, p1], 3, device=DEV)


def test_harmony_of_a_hand_made_batch():
    batch = hand_made_batch()
    h = batch.harmony()
    assert isinstance(h, Harmony) and h.sets.shape == (2, 3, 1) and h.sets.is_cuda and h.track_bits == BOUND and h.empty == "free"
    chroma = batch.chroma().cpu().numpy()
    assert h.sets.cpu().numpy().reshape(2, 3).tolist() == sets_ref(chroma, (1, 2, 3)).tolist() == [[C_MAJOR, A_MINOR | 1 << 2, 0],
                                                                                                    [0, 1 << 7 | 1 << 11, 0x231]]
    snapped = batch.harmony(snap="triad")
    assert snapped.sets.cpu().numpy().reshape(2, 3).tolist() == sets_ref(chroma, (1, 2, 3), snap="triad").tolist()
    assert snapped.sets.flatten().tolist() == [C_MAJOR, A_MINOR, 0, 0, 0x884, 0x221]       # C, Am, silence; silence, G, F
    # other tracks, finer segments
    assert batch.harmony(tracks=("Drums",)).sets.flatten().tolist() == [1, 0, 1 << 2 | 1 << 6, 0, 0, 0]
    assert batch.harmony(tracks=(1,)).sets.flatten().tolist() == [1, 1 << 9, 0, 0, 1 << 7, 0]
    for seg in (16, 8, 1):
        c = batch.chroma(seg).cpu().numpy()
        assert np.array_equal(c, chroma_ref(batch.notes.cpu().numpy(), batch.track_ptr.cpu().numpy(), 3, seg).reshape(c.shape))
        for snap in (None, "triad"):
            got = batch.harmony(seg, snap=snap)
            assert got.sets.shape == (2, 3, 32 // seg)
            assert np.array_equal(got.sets.cpu().numpy().reshape(2, -1), sets_ref(c, (1, 2, 3), snap=snap))
    halves = batch.harmony(16, snap="triad").sets[1, 2].tolist()
    assert halves == [C_MAJOR, 0x221]                                            # C and E, then F A C
    # empty = "free" / "rest" on the silent bars
    free, rest = h.chart(2, 3, DEV), Harmony(h.sets, empty="rest").chart(2, 3, DEV)
    assert free.shape == rest.shape == (6, 32) and free.dtype == torch.int32
    assert free[:, 0].tolist() == [C_MAJOR, A_MINOR | 4, FREE, FREE, 0x880, 0x231] and (free == free[:, :1]).all()
    assert rest[:, 0].tolist() == [C_MAJOR, A_MINOR | 4, 0, 0, 0x880, 0x231] and (rest == rest[:, :1]).all()


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
PROGRESSION = ["C", "Am", "F", "G", "Dm", "Em", "G7"]
# the thresholded structure of nb3_tiny holds 26 drum cells and nothing else: its cells are drawn, four at least per bar and track
MODEL_KW = {"lmd2_tiny": {}, "nb3_tiny": dict(structure_rules=StructureRules(min_active=4))}
_MODELS = {}


def model(name):
    if name not in _MODELS:
        z, cfg = load_case(name)
        gg = np.load(os.path.join(GOLDEN, f"{name}_generate.npz"), allow_pickle=False)
        vae = VAE(**cfg, device=DEV).to(DEV)
        vae.load_state_dict(state_dict_from_golden(z))
        vae.eval()
        _MODELS[name] = (vae, torch.from_numpy(gg["gen/z"]).to(DEV), cfg["n_bars"])
    return _MODELS[name]


def assert_follows(pieces, sets, tracks=(1, 2, 3), steps_per_set=32):
    """every note of `tracks` in the lists `pieces` starts in a segment whose set holds its pitch class (0 = free);
    sets [B, segments] or [segments]; returns the number of notes checked"""
    sets = np.asarray(sets)
    checked = 0
    for i, piece in enumerate(pieces):
        row = sets if sets.ndim == 1 else sets[i]
        for k in tracks:
            for (t, p, d) in piece[k]:
                s = int(row[t // steps_per_set]) if t // steps_per_set < len(row) else FREE
                assert s == 0 or (s >> (p % 12)) & 1, (i, TRACKS[k], (t, p, d), hex(s))
                checked += 1
    return checked


def breaks(pieces, sets, tracks=(1, 2, 3)):
    try:
        assert_follows(pieces, sets, tracks)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", ["lmd2_tiny", "nb3_tiny"])
def test_generate_notes_follows_a_progression(name):
    vae, zs, n_bars = model(name)
    kw = MODEL_KW[name]
    h = Harmony.from_chords(PROGRESSION[:n_bars], n_bars)
    sets = h.sets.flatten().tolist()
    with torch.no_grad():
        batch, s_tensor, tokens = generate_notes(vae, zs, harmony=h, seed=7, return_tokens=True, **kw)
        again = generate_notes(vae, zs, harmony=h, seed=7, **kw)[0]
        free = generate_notes(vae, zs, harmony=Harmony.from_chords(["N"] * n_bars, n_bars), seed=7, **kw)[0]
        plain = generate_notes(vae, zs, chord_rules=ChordRules(), seed=7, **kw)[0]
        music = generate_music(vae, zs, harmony=h, seed=7, return_tokens=True, return_note_counts=True, **kw)
    pieces = batch.tolist()
    assert assert_follows(pieces, sets) > 20
    assert again.tolist() == pieces                                              # the same seed, the same pieces
    assert [p[0] for p in free.tolist()] == [p[0] for p in pieces]               # the drums do not see the chart
    assert free.tolist() == plain.tolist() and breaks(plain.tolist(), sets)      # a free chart is no chart
    assert torch.equal(music[1], s_tensor) and torch.equal(music[2], tokens) and music[3].shape == (tokens.shape[0],)
    assert torch.equal(music[0], ops.mtp_from_tokens(tokens, s_tensor))
    # with the modes it combines with: a temperature pair, the filters, chord rules, a drawn structure
    two = Harmony.from_chords((PROGRESSION * 2)[:2 * n_bars], n_bars, per_bar=2, tracks=("Guitar", "Strings"), empty="rest")
    with torch.no_grad():
        out, s2 = generate_notes(vae, zs, harmony=two, seed=9, temperature=(0.8, 1.2), top_k=20, top_p=0.95,
                                 chord_rules=ChordRules(min_notes=1, max_notes=[14, 1, 3, 3]), structure_rules=StructureRules(min_active=2))
    assert assert_follows(out.tolist(), two.sets.flatten().tolist(), tracks=(2, 3), steps_per_set=16) > 10
    st = out.stats()
    assert (st.field("max_chord")[:, 1] <= 1).all() and (st.field("max_chord")[:, 2:] <= 3).all()
    assert int(s2[:, :, 2].sum()) >= 2 * s2.shape[0]


@pytest.mark.parametrize("name", ["lmd2_tiny", "nb3_tiny"])
def test_infill_follows_the_harmony_of_the_kept_tracks(name):
    vae, zs, n_bars = model(name)
    kw = MODEL_KW[name]
    region = region_mask(n_bars, tracks=["Guitar"])
    with torch.no_grad():
        batch = generate_notes(vae, zs, chord_rules=ChordRules(), seed=3, **kw)[0]
        h = batch.harmony(seg_steps=8, tracks=("Bass", "Strings"))
        got, s_got = infill_notes(vae, batch, region, harmony=h, seed=5, temperature=1.0, **kw)
        ref, s_ref = infill_notes(vae, batch, region, seed=5, temperature=1.0, **kw)
        rest, _ = infill_notes(vae, batch, region, harmony=Harmony(h.sets, empty="rest"), seed=5, temperature=1.0, **kw)
    assert torch.equal(s_got, s_ref)
    a, b = got.tolist(), ref.tolist()
    for k in (0, 1, 3):                                                          # the cells outside the region
        assert [p[k] for p in a] == [p[k] for p in b], TRACKS[k]
    sets = h.sets.cpu().numpy().reshape(len(a), -1)
    assert sets.shape[1] == 4 * n_bars and (sets > 0).any()
    assert assert_follows(a, sets, tracks=(2,), steps_per_set=8) > 10            # every new guitar onset is in its segment's set, or free
    # "rest": no guitar onset where bass and strings are silent, the same elsewhere
    for i, piece in enumerate(rest.tolist()):
        assert all(sets[i][t // 8] != 0 for (t, p, d) in piece[2]), i
        assert piece[2] == [r for r in a[i][2] if sets[i][r[0] // 8] != 0], i
        assert [piece[k] for k in (0, 1, 3)] == [a[i][k] for k in (0, 1, 3)]


def test_vary_song_cuts_a_harmony_into_the_windows():
    vae, zs, W = model("lmd2_tiny")
    bars, B = 2 * W + 1, 2
    rng = np.random.default_rng(4)
    songs = [[[(int(t), int(rng.integers(30, 80)), int(rng.integers(1, 12))) for t in np.sort(rng.integers(0, 32 * bars, 40 * bars))]
              for _ in range(4)] for _ in range(B)]
    song = NoteBatch.from_lists(songs, bars, device=DEV)
    shared = Harmony.from_chords(PROGRESSION[:bars], bars)
    per_song = Harmony(np.stack([shared.sets.numpy(), np.roll(shared.sets.numpy(), 1, 0)]))
    for h in (shared, per_song):
        with torch.no_grad():
            out = vary_song(vae, song, strength=0.5, seed=2, temperature=1.0, harmony=h)
        assert out.n_bars == 3 * W
        sets = h.sets.numpy().reshape(-1, bars) if h.sets.dim() == 3 else h.sets.numpy().flatten()
        assert assert_follows(out.tolist(), sets) > 40                           # (bars behind the song's end are free)
    with torch.no_grad():
        assert breaks(vary_song(vae, song, strength=0.5, seed=2, temperature=1.0, chord_rules=ChordRules()).tolist(), shared.sets.flatten().tolist())


def test_pick_takes_passes_the_harmony_on_per_take():
    vae, zs, n_bars = model("lmd2_tiny")
    z = zs[:2]
    sets = np.array([[0x091] * n_bars, [0x224] * n_bars]).reshape(2, n_bars, 1)  # C for the first latent, Dm for the second
    with torch.no_grad():
        batch, s_tensor, chosen = pick_takes(vae, z, 3, lambda st: st.field("n_notes").sum(1).float(), harmony=Harmony(sets), seed=11,
                                             temperature=1.0)
        shared, _, _ = pick_takes(vae, z, 3, lambda st: st.field("n_notes").sum(1).float(), harmony=Harmony(sets[0]), seed=11, temperature=1.0)
    assert (chosen // 3).tolist() == [0, 1] and s_tensor.shape[0] == 2
    assert assert_follows(batch.tolist(), sets.reshape(2, n_bars)) > 10
    assert assert_follows(shared.tolist(), sets[0].flatten()) > 10
