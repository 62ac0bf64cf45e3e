"""Note statistics on the device (csrc/stats.hip: `ops.note_stats` / `ops.notes_select`, `NoteBatch.stats` / `select`,
`NoteStats`, `pick_takes`) against the numpy restatement of tests/stats_util.py, which tests/test_stats_abi.py ties to a piece
computed by hand and to the reference's recorded notes.  The counts are integers and every comparison of them is exact; the
derived measures are compared with their float64 restatement."""
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import ChordRules, NoteBatch, NoteStats, StructureRules, encode_notes, generate_notes, pick_takes
from polyphemus_amd.model import VAE
from stats_util import FIELDS, derived_ref, select_ref, stats_ref
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -123456789
PAD = 64
F = {name: i for i, name in enumerate(FIELDS)}


def hand_made(B, n_bars, seed=0):
    """pieces as lists.  Piece 0 by hand: an empty track, a track of one row, one of more than 64 and one of more than 256
    rows (the lanes' stride); in the third track 20 onsets in one cell, onsets at step 0 and at the last step (bit 31 of the last
    word), a note that ends exactly at the end of the piece and one that is cut there, a note across the first bar line,
    pitches -3 and 200, durations 0, 1, 96, 97 and 500, one pitch twice in a cell.  Piece 1 is empty, the others are drawn."""
    L = 32 * n_bars
    rng = np.random.default_rng(seed)

    def drawn(n):
        times = np.sort(rng.integers(0, L, n))
        return [(int(t), int(rng.integers(-5, 135)), int(rng.integers(-2, 110))) for t in times]

    pieces = [[[], [], [], []] for _ in range(B)]
    hard = ([(0, 36, 0), (0, -3, 1)] + [(3, 40 + j, 1 + j % 5) for j in range(20)] + [(7, 60, 2), (7, 60, 3), (9, 200, 96), (11, 70, 97)]
            + [(30, 52, 6), (L - 4, 50, 4), (L - 2, 51, 10), (L - 1, 127, 500), (L - 1, 0, 1)])
    pieces[0][1] = [(5, 41, 3)]
    pieces[0][2] = sorted(hard + drawn(70 - len(hard)), key=lambda r: r[0])
    pieces[0][3] = drawn(300)
    for i in range(2, B):
        for k in range(4):
            pieces[i][k] = drawn(int(rng.integers(0, 40)))
    return pieces


def as_batch(pieces):
    rows = [r for piece in pieces for track in piece for r in track]
    ptr = np.cumsum([0] + [len(track) for piece in pieces for track in piece]).astype(np.int32)
    return np.asarray(rows, np.int32).reshape(-1, 3), ptr


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_stats(notes, ptr, n_bars, M=None):
    """pm_note_stats through the raw binding, every output pre-filled with a sentinel and followed by PAD sentinel words:
    (track, pitch_class, onsets, sounding) as numpy after the check that the pads are intact"""
    T = len(ptr) - 1
    M = len(notes) if M is None else M
    nd, pd = dev(notes), dev(ptr)
    sizes = (12 * T, 12 * T, n_bars * T, n_bars * T)
    outs = [torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for n in sizes]
    _lib.call("pm_note_stats", nd.data_ptr() if M else None, pd.data_ptr(), T // 4, n_bars, M, *(o.data_ptr() for o in outs),
              _lib.stream())
    res = []
    for o, n in zip(outs, sizes):
        a = o.cpu().numpy()
        assert (a[n:] == SENTINEL).all()
        res.append(a[:n].reshape(T, -1))
    return res


def assert_stats_equal_ref(notes, ptr, n_bars, M=None):
    want = stats_ref(notes[:M], ptr, n_bars)
    got = raw_stats(notes, ptr, n_bars, M)
    for name, g, w in zip(("track", "pitch_class", "onsets", "sounding"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist())
    # ... and through the wrapper
    wrapped = ops.note_stats(dev(notes[:M]), dev(ptr), n_bars)
    assert all(t.dtype == torch.int32 and t.is_cuda and np.array_equal(t.cpu().numpy(), w) for t, w in zip(wrapped, want))
    return want


@pytest.mark.parametrize("B,n_bars", [(1, 1), (3, 2), (5, 3)])
def test_hand_made_batches_equal_the_restatement(B, n_bars):
    """L = 32, 64 and 96 steps: one chunk of the scan half full, one full, two with the second half full"""
    pieces = hand_made(B, n_bars)
    notes, ptr = as_batch(pieces)
    track, pc, onsets, sounding = assert_stats_equal_ref(notes, ptr, n_bars)
    L = 32 * n_bars
    assert track[0].tolist() == [0, 0, 128, -1] + [0] * 8                               # the empty track, written all the same
    assert track[1].tolist() == [1, 1, 41, 41, 1, 1, 3, 3, 0, 1, 1, 0]
    assert track[2, F["n_notes"]] == 70 and track[3, F["n_notes"]] == 300 and not track[:, F["out_of_range"]].any()
    assert track[2, F["max_chord"]] >= 20 and track[2, F["pitch_min"]] == 0 and track[2, F["pitch_max"]] == 127
    assert onsets[2, 0] & 1 and onsets[2, n_bars - 1] < 0 and sounding[2, n_bars - 1] < 0  # step 0; bit 31 of the last word
    if B > 1:
        assert track[4:8].tolist() == [[0, 0, 128, -1] + [0] * 8] * 4 and not pc[4:8].any() and not onsets[4:8].any()
    # two calls write the same bytes
    again = raw_stats(notes, ptr, n_bars)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (track, pc, onsets, sounding)))


def test_row_order_does_not_matter():
    n_bars = 3
    pieces = hand_made(4, n_bars, seed=5)
    notes, ptr = as_batch(pieces)
    rng = np.random.default_rng(1)
    shuffled = notes.copy()
    for tr in range(len(ptr) - 1):
        shuffled[ptr[tr]:ptr[tr + 1]] = notes[ptr[tr]:ptr[tr + 1]][rng.permutation(ptr[tr + 1] - ptr[tr])]
    assert not np.array_equal(shuffled, notes)
    a, b = raw_stats(notes, ptr, n_bars), raw_stats(shuffled, ptr, n_bars)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert_stats_equal_ref(shuffled, ptr, n_bars)


def test_rows_outside_the_piece_are_counted_and_nothing_else():
    n_bars = 2
    L = 32 * n_bars
    inside = [(0, 60, 4), (L - 1, 62, 4)]
    pieces = [[inside + [(-1, 1, 50), (L, 2, 50)], [(L, 3, 1)], [(-1, 4, 1), (-(1 << 31), 5, 1), ((1 << 31) - 1, 6, 1)], []],
              [inside, [], [], []]]
    notes, ptr = as_batch(pieces)
    track, pc, onsets, sounding = assert_stats_equal_ref(notes, ptr, n_bars)
    assert track[:, F["out_of_range"]].tolist() == [2, 1, 3, 0, 0, 0, 0, 0]
    # but for that count, track 0 of piece 0 reads as track 0 of piece 1; tracks of such rows alone read as empty
    assert track[0, :11].tolist() == track[4, :11].tolist() and np.array_equal(pc[0], pc[4])
    assert np.array_equal(onsets[0], onsets[4]) and np.array_equal(sounding[0], sounding[4])
    assert track[1, :11].tolist() == track[2, :11].tolist() == [0, 0, 128, -1] + [0] * 7 and not pc[1:4].any()
    nb = NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), n_bars)
    assert nb.stats().field("out_of_range").sum().item() == 6                           # check=False: counted
    with pytest.raises(ValueError, match="6 rows out of range"):
        nb.stats(check=True)
    with pytest.raises(ValueError, match="6 rows out of range"):
        ops.note_stats(nb.notes, nb.track_ptr, n_bars, check=True)


def test_track_ptr_is_clamped_and_rows_behind_it_are_not_read():
    """sentinel rows behind track_ptr[4B] belong to no track; entries below 0, beyond M and below their predecessor are
    clamped into [0, M] as pm_tokens_from_notes clamps them, and M itself may be smaller than the buffer"""
    n_bars = 2
    notes, ptr = as_batch(hand_made(3, n_bars, seed=2))
    M = len(notes)
    padded = np.concatenate([notes, np.full((40, 3), SENTINEL, np.int32)])
    assert_stats_equal_ref(padded, ptr, n_bars)                                         # M = the buffer's rows
    assert_stats_equal_ref(padded, ptr, n_bars, M=M)
    bad = ptr.copy()
    bad[1], bad[3], bad[6], bad[9], bad[12] = -7, M + 50, 2, (1 << 31) - 1, M + 1
    want = assert_stats_equal_ref(padded, bad, n_bars, M=M)
    assert want[0][:, F["out_of_range"]].sum() == 0                                      # no sentinel row was taken for a note
    assert_stats_equal_ref(padded, bad, n_bars, M=M - 13)
    # no rows at all
    assert_stats_equal_ref(np.zeros((0, 3), np.int32), np.zeros(9, np.int32), n_bars)


def test_the_longest_piece_and_one_bar_more():
    """n_bars = 64: the whole LDS of a workgroup holds the counters; 65 is refused before any launch"""
    n_bars, rng = 64, np.random.default_rng(9)
    L = 32 * n_bars
    pieces = [[[(int(t), int(rng.integers(0, 128)), int(rng.integers(1, 97))) for t in np.sort(rng.integers(0, L, n))]
               for n in (0, 1, 90, 400)] for _ in range(2)]
    pieces[1][2] += [(L - 1, 5, 9), (L - 96, 6, 96), (L - 95, 7, 96)]
    notes, ptr = as_batch(pieces)
    track, _, onsets, sounding = assert_stats_equal_ref(notes, ptr, n_bars)
    assert onsets[6, 63] < 0 and sounding[6, 63] == -1 and track[7, F["sounding_steps"]] > 1500
    with pytest.raises(ValueError, match="n_bars"):
        ops.note_stats(dev(notes), dev(ptr), 65)
    outs = [torch.full((12 * 8,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2)]
    outs += [torch.full((65 * 8,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(2)]
    nd, pd = dev(notes), dev(ptr)
    rc = _lib.lib().pm_note_stats(nd.data_ptr(), pd.data_ptr(), 2, 65, len(notes), *(o.data_ptr() for o in outs), _lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and all((o == SENTINEL).all() for o in outs)


# ---- derived measures ---------------------------------------------------------------------------------------------------------
# fp32 against float64.  polyphony, polyphony_rate, scale_consistency and groove_consistency are one division of two integers
# below 2^24 (exact in fp32) and at most one subtraction: two roundings of a value <= 96.  empty_beat_rate is a mean of at most
# 256 zeros and ones and a subtraction.  pitch_class_entropy is the longest: 12 divisions, 12 log2 (1 - 2 ulp on the device),
# 12 products, 11 additions and a negation, 48 operations, above the 40 the other measures stay under; its terms are below
# 0.54 in magnitude and its partial sums below log2(12) = 3.59, so the error is below 12 * 0.54 * 4 * 2^-24 + 11 * 3.59 * 2^-24
# = 3.9e-6.  All of them are within the absolute tolerance 1e-5.
ATOL = 1e-5


@pytest.mark.parametrize("B,n_bars,resolution", [(1, 1, 8), (3, 2, 8), (5, 3, 4), (2, 2, 32), (2, 2, 1)])
def test_derived_measures_equal_the_float64_restatement(B, n_bars, resolution):
    notes, ptr = as_batch(hand_made(B, n_bars, seed=B))
    nb = NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), n_bars, resolution)
    st = nb.stats()
    assert isinstance(st, NoteStats) and st.n_bars == n_bars and st.resolution == resolution
    assert st.track.shape == (B, 4, 12) and st.pitch_class.shape == (B, 4, 12) and st.onsets.shape == st.sounding.shape == (B, 4, n_bars)
    raw = stats_ref(notes, ptr, n_bars)
    for t, w in zip((st.track, st.pitch_class, st.onsets, st.sounding), raw):
        assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy().reshape(w.shape), w)
    assert torch.equal(st.field("max_chord"), st.track[..., 10])
    want = derived_ref(*raw, n_bars, resolution)
    for name, w in want.items():
        got = getattr(st, name)()
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == w.shape, name
        err = np.abs(got.cpu().numpy().astype(np.float64) - w).max()
        print(f"{name}: max abs error {err:.3e}")
        assert err <= ATOL, (name, err)
    assert want["pitch_class_entropy"].max() > 3 and want["polyphony"].max() > 2            # (the measures are not trivial here)
    if n_bars == 1:
        assert (st.groove_consistency() == 1).all()


# ---- the golden model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    """(vae in eval mode, latents, n_bars) of the smaller golden case"""
    z, cfg = load_case("lmd2_tiny")
    gg = np.load(os.path.join(GOLDEN, "lmd2_tiny_generate.npz"), allow_pickle=False)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    return vae, torch.from_numpy(gg["gen/z"]).to(DEV), cfg["n_bars"]


@pytest.fixture(scope="module")
def take(model):
    """a sampled NoteBatch whose Bass track holds at most one note per cell"""
    vae, zs, _ = model
    with torch.no_grad():
        return generate_notes(vae, zs, chord_rules=ChordRules(max_notes=[14, 1, 14, 14]), seed=3)[0]


def lists_as_batch(pieces):
    return as_batch([[list(track) for track in piece] for piece in pieces])


def test_generated_takes_equal_the_restatement_on_their_lists(model, take):
    vae, zs, n_bars = model
    with torch.no_grad():
        argmax = generate_notes(vae, zs)[0]
    for batch in (argmax, take):
        notes, ptr = lists_as_batch(batch.tolist())
        st = batch.stats(check=True)
        for t, w in zip((st.track, st.pitch_class, st.onsets, st.sounding), stats_ref(notes, ptr, n_bars)):
            assert np.array_equal(t.cpu().numpy().reshape(w.shape), w)
        assert st.field("n_notes").sum().item() == batch.totals[0].item()
    st = take.stats()
    assert st.field("n_notes")[:, 1].sum().item() > 0 and (st.field("max_chord")[:, 1] <= 1).all()   # what the rules guarantee


# ---- select -------------------------------------------------------------------------------------------------------------------
def raw_select(notes, ptr, index, cap):
    """pm_notes_select through the raw binding, every output in front of PAD sentinel words and out_notes pre-filled:
    (out_notes [cap,3], out_track_ptr, totals, status) as numpy after the check that the pads are intact"""
    B, M, K = (len(ptr) - 1) // 4, len(notes), len(index)
    sizes = (3 * cap, 4 * K + 1, 2, B + 16 * K, 2)
    out, out_ptr, totals, scratch, status = (torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for n in sizes)
    nd, pd, xd = dev(notes), dev(ptr), dev(np.asarray(index, np.int32))                    # (alive until the results are read)
    _lib.call("pm_notes_select", nd.data_ptr() if M else None, pd.data_ptr(), B, M, xd.data_ptr(), K, out.data_ptr() if cap else None,
              cap, out_ptr.data_ptr(), totals.data_ptr(), scratch.data_ptr(), status.data_ptr(), _lib.stream())
    res = []
    for o, n in zip((out, out_ptr, totals, scratch, status), sizes):
        a = o.cpu().numpy()
        assert (a[n:] == SENTINEL).all()
        res.append(a[:n])
    return res[0].reshape(cap, 3), res[1], res[2].tolist(), res[4].tolist()


SELECT_B = 5
INDEXES = {"one": [3], "one-empty": [1], "permutation": [4, 0, 2, 1, 3], "subset-with-the-empty-piece": [2, 1, 0], "identity": [0, 1, 2, 3, 4]}


@pytest.mark.parametrize("kind", list(INDEXES))
def test_select_equals_the_restatement(kind):
    index = INDEXES[kind]
    pieces = hand_made(SELECT_B, 3, seed=4)
    notes, ptr = as_batch(pieces)
    want, want_ptr, want_totals, want_status = select_ref(notes, ptr, index)
    assert want_status == [0, 0] and want_totals[0] == sum(len(t) for i in index for t in pieces[i])
    for cap in (len(notes), len(want), len(want) + 5):
        out, out_ptr, totals, status = raw_select(notes, ptr, index, cap)
        assert np.array_equal(out_ptr, want_ptr) and totals == want_totals and status == [0, 0]
        assert np.array_equal(out[:len(want)], want) and (out[len(want):] == SENTINEL).all()   # rows from M' on are untouched
    nb = NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), 3, resolution=4)
    lists = nb.tolist()
    for idx in (index, torch.tensor(index, dtype=torch.int32, device=DEV), torch.tensor(index, dtype=torch.int64, device=DEV)):
        sel = nb.select(idx)
        assert isinstance(sel, NoteBatch) and sel.n_bars == 3 and sel.resolution == 4 and sel.notes.is_cuda
        assert sel.notes.dtype == sel.track_ptr.dtype == sel.totals.dtype == torch.int32 and sel.track_ptr.shape == (4 * len(index) + 1,)
        assert sel.tolist() == [lists[i] for i in index] and sel.totals.tolist() == want_totals
    assert lists == [[[tuple(r) for r in t] for t in p] for p in pieces]


def test_select_counts_bad_entries_and_never_follows_them():
    pieces = hand_made(SELECT_B, 2, seed=6)
    notes, ptr = as_batch(pieces)
    nb = NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), 2)
    lists = nb.tolist()
    empty = [[], [], [], []]
    for index, want_status, want_lists in (([2, 7, 0, 2], [1, 1], [lists[2], empty, lists[0], empty]),
                                            ([-1, SELECT_B, 3], [2, 0], [empty, empty, lists[3]]),
                                            ([4, 4, 4, 0, 0], [0, 3], [lists[4], empty, empty, lists[0], empty])):
        want, want_ptr, want_totals, status = select_ref(notes, ptr, index)
        assert status == want_status
        out, out_ptr, totals, got_status = raw_select(notes, ptr, index, len(notes))
        assert got_status == want_status and np.array_equal(out_ptr, want_ptr) and totals == want_totals
        assert np.array_equal(out[:len(want)], want) and (out[len(want):] == SENTINEL).all()
        n, p, t, s = ops.notes_select(nb.notes, nb.track_ptr, index, check=False)
        assert s.dtype == torch.int32 and s.is_cuda and s.tolist() == want_status and t.tolist() == want_totals
        assert nb.select(index, check=False).tolist() == want_lists
        for idx in (index, torch.tensor(index, device=DEV)):
            with pytest.raises(ValueError, match=f"{want_status[0]} entries outside .* {want_status[1]} entries that repeat"):
                nb.select(idx)
    big = torch.tensor([1 << 40, 1, -(1 << 40)], dtype=torch.int64, device=DEV)            # beyond int32: out of range
    assert ops.notes_select(nb.notes, nb.track_ptr, big, check=False)[3].tolist() == [2, 0]
    # a capacity below M': nothing at or beyond it is written
    want, want_ptr, want_totals, _ = select_ref(notes, ptr, [0, 2])
    cap = len(want) - 7
    out, out_ptr, totals, _ = raw_select(notes, ptr, [0, 2], cap)
    assert np.array_equal(out, want[:cap]) and np.array_equal(out_ptr, want_ptr) and totals == want_totals
    # a track_ptr that breaks the contract is clamped, as in the statistics
    bad = ptr.copy()
    bad[2], bad[5], bad[11] = -4, len(notes) + 9, 1
    want, want_ptr, want_totals, _ = select_ref(notes, bad, [2, 0, 1])
    out, out_ptr, totals, status = raw_select(notes, bad, [2, 0, 1], len(want) + 3)
    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == SENTINEL).all() and np.array_equal(out_ptr, want_ptr)
    assert totals == want_totals and status == [0, 0]


def test_selected_pieces_encode_as_the_same_pieces_from_lists(model, take):
    vae, _, n_bars = model
    index = [5, 0, 6, 2]
    sel = take.select(index)
    again = NoteBatch.from_lists([take.tolist()[i] for i in index], n_bars, device=DEV)
    M = int(again.totals[0])
    assert torch.equal(sel.track_ptr, again.track_ptr) and torch.equal(sel.notes[:M], again.notes) and torch.equal(sel.totals, again.totals)
    g1, g2 = sel.to_graph(), again.to_graph()
    assert torch.equal(g1.tokens, g2.tokens) and torch.equal(g1.s_tensor, g2.s_tensor) and torch.equal(g1.edge_index, g2.edge_index)
    (mu1, lv1), (mu2, lv2) = encode_notes(vae, sel), encode_notes(vae, again)
    assert torch.equal(mu1, mu2) and torch.equal(lv1, lv2) and mu1.shape[0] == len(index)


# ---- pick_takes ---------------------------------------------------------------------------------------------------------------
def test_pick_takes_keeps_the_best_take_of_every_latent(model):
    vae, zs, n_bars = model
    B, takes = 2, 4
    z = zs[:B]
    kw = dict(chord_rules=ChordRules(max_notes=[14, 1, 14, 14]), structure_rules=StructureRules(), seed=11)
    with torch.no_grad():
        every, s_every = generate_notes(vae, z.repeat_interleave(takes, 0), **kw)
    lists = every.tolist()
    assert len(lists) == B * takes and len({str(p) for p in lists}) > B                    # the takes of a latent differ
    keys = {"fewest-bass-notes-at-once": lambda st: -st.track[:, 1, 9].float(),
            "most-notes": lambda st: st.field("n_notes").sum(1).float(),
            "groove": lambda st: st.groove_consistency().mean(1) - st.empty_beat_rate(),
            "constant": lambda st: torch.zeros(B * takes, device=DEV),
            "nan-first": lambda st: torch.tensor([float("nan")] + [1.0] * (B * takes - 1), device=DEV),
            "half": lambda st: st.field("n_notes").sum(1).half(),
            "all-nan": lambda st: torch.full((B * takes,), float("nan"), device=DEV)}
    for name, key in keys.items():
        with torch.no_grad():
            batch, s_tensor, chosen = pick_takes(vae, z, takes, key, **kw)
        score = key(every.stats()).float().cpu().numpy().astype(np.float64)
        score[np.isnan(score)] = -np.inf
        want = [int(np.argmax(score[g * takes:(g + 1) * takes])) + g * takes for g in range(B)]   # (the first of equal maxima)
        assert chosen.dtype == torch.int64 and chosen.is_cuda and chosen.tolist() == want, name
        assert batch.tolist() == [lists[r] for r in want] and torch.equal(s_tensor, s_every[chosen]), name
        assert batch.n_bars == n_bars and batch.track_ptr.shape == (4 * B + 1,)
        if name == "constant" or name == "all-nan":
            assert want == [0, 4]
        if name == "nan-first":
            assert want == [1, 4]
    assert (every.stats().field("max_chord")[:, 1] <= 1).all()
    # takes = 1: the call itself
    with torch.no_grad():
        batch, s_tensor, chosen = pick_takes(vae, z, 1, keys["most-notes"], **kw)
        one, s_one = generate_notes(vae, z, **kw)
    assert chosen.tolist() == [0, 1] and batch.tolist() == one.tolist() and torch.equal(s_tensor, s_one)
    # a given structure is repeated with the latents
    with torch.no_grad():
        s_cond = s_one.clone()
        batch, s_tensor, chosen = pick_takes(vae, z, 2, keys["most-notes"], s_cond=vae.decoder._structure_from_binary(s_cond),
                                             s_tensor_cond=s_cond, chord_rules=ChordRules(), seed=5)
    assert torch.equal(s_tensor, s_one) and (chosen // 2).tolist() == [0, 1]
    for key, what in ((lambda st: torch.zeros(B * takes - 1, device=DEV), "key must return"), (lambda st: torch.zeros(B, takes, device=DEV), "key must return"),
                      (lambda st: st.track[:, 1, 9], "key must return"), (lambda st: torch.zeros(B * takes), "key must return"),
                      (lambda st: [0.0] * (B * takes), "key must return")):
        with pytest.raises(ValueError, match=what):
            with torch.no_grad():
                pick_takes(vae, z, takes, key, **kw)
