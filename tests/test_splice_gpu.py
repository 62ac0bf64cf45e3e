"""Note splicing on the device (csrc/splice.hip: `ops.notes_splice`, `NoteBatch.windows` / `join`, `generate.encode_song` /
`vary_song`) against the restatement of tests/splice_util.py, which tests/test_splice_cpu.py ties to cases computed by hand.
Everything is an integer (or, for the latents, the same arithmetic on the same input): every comparison is exact."""
import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import NoteBatch, WindowIndex, encode_notes, encode_song, vary_notes, vary_song
from polyphemus_amd.model import VAE
from notes_util import as_lists, load_notes
from splice_util import filter_ref, join_np, splice_ref, transposed, window_acts, windows_np
from util import load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -123456789
PAD = 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def flat(pieces):
    rows = [r for piece in pieces for track in piece for r in track]
    ptr = np.cumsum([0] + [len(track) for piece in pieces for track in piece]).astype(np.int32)
    return np.asarray(rows, np.int32).reshape(-1, 3), ptr


def batch_of(pieces, n_bars):
    """a NoteBatch of the lists as they are: no sorting, no check of the times"""
    notes, ptr = flat(pieces)
    return NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), n_bars)


def lists(nb):
    return [[[tuple(r) for r in track] for track in piece] for piece in nb.tolist()]


def raw_splice(notes, ptr, src_bars, segments, seg_ptr, out_bars, shift=None, rule=0, cap=None):
    """pm_notes_splice through the raw binding, every output in front of PAD sentinel words and out_notes pre-filled:
    (out_notes [cap,3], out_track_ptr, totals, keep, status) as numpy after the check that the pads are intact"""
    B, M, K = (len(ptr) - 1) // 4, len(notes), len(seg_ptr) - 1
    segments = np.asarray(segments, np.int32).reshape(-1, 4)
    S = len(segments)
    cap = M if cap is None else cap
    sizes = (3 * cap, 4 * K + 1, 2, K, 24 * K, 4)
    out, out_ptr, totals, keep, scratch, status = (torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device=DEV) for n in sizes)
    nd, pd, sd, qd = dev(notes), dev(ptr), dev(segments), dev(np.asarray(seg_ptr, np.int32))      # (alive until the results are read)
    hd = None if shift is None else dev(np.asarray(shift, np.int32))
    _lib.call("pm_notes_splice", nd.data_ptr() if M else None, pd.data_ptr(), B, src_bars, M, sd.data_ptr() if S else None, S,
              qd.data_ptr(), K, out_bars, None if hd is None else hd.data_ptr(), rule, out.data_ptr() if cap else None, cap,
              out_ptr.data_ptr(), totals.data_ptr(), keep.data_ptr(), scratch.data_ptr(), status.data_ptr(), _lib.stream())
    res = []
    for o, n in zip((out, out_ptr, totals, keep, scratch, status), sizes):
        a = o.cpu().numpy()
        assert (a[n:] == SENTINEL).all()
        res.append(a[:n])
    return res[0].reshape(cap, 3), res[1], res[2].tolist(), res[3].tolist(), res[5].tolist()


def assert_splice_equals_ref(notes, ptr, src_bars, segments, seg_ptr, out_bars, shift=None, rule=0, cap=None):
    want, want_ptr, want_totals, want_keep, want_status = splice_ref(notes, ptr, src_bars, segments, seg_ptr, out_bars, shift, bool(rule))
    cap = len(notes) if cap is None else cap
    out, out_ptr, totals, keep, status = raw_splice(notes, ptr, src_bars, segments, seg_ptr, out_bars, shift, rule, cap)
    n = min(cap, len(want))
    assert np.array_equal(out_ptr, want_ptr) and totals == want_totals and keep == want_keep
    assert np.array_equal(out[:n], want[:n]) and (out[n:] == SENTINEL).all()                # rows from M' on are untouched
    assert status == want_status + [max(len(want) - cap, 0), 0]
    return want, want_ptr, want_totals, want_keep, status


# ---- sliding windows ----------------------------------------------------------------------------------------------------------
def chord(t, n, base=30):
    return [(t, base + (7 * j) % 50, 1 + j) for j in range(n)]


def songs(seed=0):
    """two songs of 5 bars, every track sorted by time: a timestep of 16 notes, a note at the first and at the last step, a
    note longer than what is left of its window, an empty track, a track of one note"""
    rng = np.random.default_rng(seed)

    def drawn(n, bars=5):
        return [(int(t), int(rng.integers(20, 100)), int(rng.integers(1, 40))) for t in np.sort(rng.integers(0, 32 * bars, n))]

    a = [sorted(drawn(40) + chord(40, 16) + [(0, 36, 4), (159, 38, 9)], key=lambda r: r[0]), drawn(25) + [(159, 50, 200)], [], [(64, 60, 96)]]
    b = [drawn(30), [], drawn(12, bars=3), drawn(50)]
    return [a, b]


def alternating():
    """130 rows that lie by turns inside the window of bars 1-2 (times that do not decrease there) and outside it: the rows
    that go along sit in three chunks of 64 lanes and have to come out in this order"""
    return [(32 + (i // 2) * 63 // 64, 40 + i % 50, 1 + i % 7) if i % 2 == 0 else ((0, 1, 1), (100, 2, 2), (159, 3, 3))[i // 2 % 3] for i in range(130)]


def unsorted_songs():
    """the songs with a track in falling order, the alternating track, and rows whose time lies outside the song"""
    a, b = songs()
    a = [a[0], a[1][::-1], alternating(), a[3] + [(-5, 1, 1), (160, 2, 2), (1 << 30, 3, 3), (-(1 << 31), 4, 4)]]
    b = [b[0] + [(161, 5, 5)], b[1], b[2], b[3][::-1]]
    return [a, b]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("song_bars", [None, [5, 3]], ids=["whole", "5-and-3-bars"])
def test_windows_equal_the_host_route(stride, song_bars):
    for pieces, nb in ((songs(), NoteBatch.from_lists(songs(), 5, device=DEV)), (unsorted_songs(), batch_of(unsorted_songs(), 5))):
        want, song, start = windows_np(pieces, 2, stride, song_bars, total_bars=5)
        got, index = nb.windows(2, stride=stride, song_bars=song_bars)
        assert isinstance(got, NoteBatch) and got.n_bars == 2 and got.resolution == nb.resolution and isinstance(index, WindowIndex)
        assert lists(got) == want
        assert index.song.tolist() == song and index.start.tolist() == start and index.shift.tolist() == [0] * len(want)
        assert all(t.dtype == torch.int32 and t.is_cuda for t in (got.notes, got.track_ptr, got.totals, index.song, index.start, index.shift))
        assert got.notes.shape == (nb.notes.shape[0] * (2 // stride), 3) and got.track_ptr.shape == (4 * len(want) + 1,)
        n = sum(len(t) for w in want for t in w)
        assert got.totals[0].item() == got.track_ptr[-1].item() == n
        # the raw entry on the same segments, against the restatement
        segments = [(b, s, 0, 2) for b, s in zip(song, start)]
        notes, ptr = flat(pieces)
        rows, _, totals, _, _ = assert_splice_equals_ref(notes, ptr, 5, segments, list(range(len(segments) + 1)), 2, cap=n + 3)
        assert np.array_equal(rows, flat(want)[0]) and totals[0] == n
        assert got.totals.tolist() == totals


def test_the_order_of_a_track_is_kept_across_chunks():
    pieces = unsorted_songs()
    got, _ = batch_of(pieces, 5).windows(2, stride=1)
    inside = [(t - 32, p, d) for (t, p, d) in alternating() if 32 <= t < 96]
    assert len(inside) == 65 and lists(got)[1][2] == inside                                # window 1 of song 0, the third track
    assert lists(got)[0][1] == [(t, p, d) for (t, p, d) in pieces[0][1] if t < 64]            # the falling track stays falling
    assert lists(got)[0][1][0][0] > lists(got)[0][1][-1][0]


def test_windows_read_as_the_host_cut_windows_by_the_encoder():
    """a timestep of 16 notes: the slots, and which two notes are dropped, follow the order of the rows"""
    pieces = songs()
    nb = NoteBatch.from_lists(pieces, 5, device=DEV)
    got, _ = nb.windows(2, stride=1)
    want = NoteBatch.from_lists(windows_np(pieces, 2, 1, total_bars=5)[0], 2, device=DEV)
    M = int(want.totals[0])
    assert torch.equal(got.track_ptr, want.track_ptr) and torch.equal(got.notes[:M], want.notes) and torch.equal(got.totals, want.totals)
    s1, t1, info1 = ops.tokens_from_notes(got.notes, got.track_ptr, 2)
    s2, t2, info2 = ops.tokens_from_notes(want.notes, want.track_ptr, 2)
    assert torch.equal(s1, s2) and torch.equal(t1, t2) and info1 == info2 and info1["dropped"] >= 2 * 2    # the chord lies in two windows


def test_song_lengths_as_a_tensor_are_not_read():
    pieces = songs()
    nb = NoteBatch.from_lists(pieces, 5, device=DEV)
    for bars in ([5, 3], [1, 5], [0, 2]):
        got, index = nb.windows(2, stride=1, song_bars=torch.tensor(bars, device=DEV))
        want = []
        for b in range(2):
            fit = windows_np(pieces[b:b + 1], 2, 1, song_bars=bars[b:b + 1])[0]
            want += [(b, w) for w in fit] + [(-1, [[], [], [], []])] * (4 - len(fit))
        assert lists(got) == [w for _, w in want] and index.song.tolist() == [b for b, _ in want]
        assert index.start.tolist() == [0, 1, 2, 3] * 2
    # with the filter the windows that do not fit go like every silent window
    got, index = nb.windows(1, song_bars=torch.tensor([2, 1], dtype=torch.int32, device=DEV), filter="reference")
    fit, song, start = windows_np(pieces, 1, 1, song_bars=[2, 1])
    keep = [filter_ref(window_acts(w, 1)) for w in fit]
    assert any(keep) and index.song.tolist() == [b for b, k in zip(song, keep) if k] and index.start.tolist() == [s for s, k in zip(start, keep) if k]
    assert lists(got) == [w for w, k in zip(fit, keep) if k]


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    empty = [[], [], [], []]
    # no rows at all: three silent windows, a notes buffer without rows
    nb = batch_of([empty], 3)
    got, index = nb.windows(1)
    assert lists(got) == [empty] * 3 and got.notes.shape == (0, 3) and got.totals.tolist() == [0, 0] and index.start.tolist() == [0, 1, 2]
    assert lists(nb.join([[0, -1]])) == [empty]
    assert_splice_equals_ref(np.zeros((0, 3), np.int32), np.zeros(5, np.int32), 3, [(0, 0, 0, 1)], [0, 1], 1, rule=1)
    # K = 1: the whole song is the window, and a song with an empty track
    pieces = songs()
    nb = NoteBatch.from_lists(pieces[:1], 5, device=DEV)
    got, index = nb.windows(5)
    assert lists(got) == pieces[:1] and index.song.tolist() == [0] and index.start.tolist() == [0] and got.totals.tolist() == nb.totals.tolist()
    # an output piece without a segment, between two that have one; no segments at all
    notes, ptr = flat(pieces)
    want = assert_splice_equals_ref(notes, ptr, 5, [(0, 0, 0, 2), (1, 3, 0, 2)], [0, 1, 1, 2], 2, rule=1)
    assert want[1][4:9].tolist() == [want[1][4]] * 5 and want[3][1] == 0
    assert_splice_equals_ref(notes, ptr, 5, np.zeros((0, 4), np.int32), [0, 0, 0], 2, rule=1)
    # two calls write the same bytes
    a = raw_splice(notes, ptr, 5, [(0, 0, 0, 2), (1, 3, 0, 2)], [0, 1, 1, 2], 2, rule=1)
    b = raw_splice(notes, ptr, 5, [(0, 0, 0, 2), (1, 3, 0, 2)], [0, 1, 1, 2], 2, rule=1)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- what is counted is not followed ----------------------------------------------------------------------------------------------
BAD_SEGMENTS = {"piece beyond the batch": (2, 0, 0, 2), "negative piece": (-1, 0, 0, 2), "negative bar": (0, -1, 0, 2),
                "beyond the source": (0, 4, 0, 2), "beyond the output": (0, 0, 1, 2), "negative output bar": (0, 0, -1, 1),
                "no bars": (0, 0, 0, 0), "negative bars": (0, 1, 0, -1), "huge": (0, (1 << 31) - 1, 0, (1 << 31) - 1)}


@pytest.mark.parametrize("kind", list(BAD_SEGMENTS))
def test_a_bad_segment_is_counted_and_copies_nothing(kind):
    notes, ptr = flat(unsorted_songs())
    good, bad = (1, 1, 0, 2), BAD_SEGMENTS[kind]
    want = assert_splice_equals_ref(notes, ptr, 5, [bad, good, bad], [0, 1, 3], 2)
    alone = splice_ref(notes, ptr, 5, [good], [0, 0, 1], 2)
    assert want[4][:2] == [2, 0] and np.array_equal(want[0], alone[0]) and np.array_equal(want[1], alone[1])
    nb = batch_of(unsorted_songs(), 5)
    args = (nb.notes, nb.track_ptr, 5, dev(np.asarray([bad, good, bad], np.int32)), dev(np.asarray([0, 1, 3], np.int32)), 2)
    with pytest.raises(ValueError, match="segments: 2 not followed"):
        ops.notes_splice(*args)
    out, out_ptr, totals, keep, status = ops.notes_splice(*args, check=False)
    assert status.tolist() == [2, 0, 0, 0] and status.is_cuda and totals.tolist() == want[2] and keep.tolist() == [1, 1]
    assert np.array_equal(out[:len(want[0])].cpu().numpy(), want[0]) and np.array_equal(out_ptr.cpu().numpy(), want[1])


def test_overlapping_outputs_and_a_bad_seg_ptr():
    notes, ptr = flat(unsorted_songs())
    # the second segment starts in front of the end of the first; the third starts at it
    want = assert_splice_equals_ref(notes, ptr, 5, [(0, 0, 0, 2), (0, 2, 1, 1), (1, 0, 2, 1)], [0, 3], 3)
    assert want[4][:2] == [1, 0]
    # ... and an order that goes backwards in the output
    want = assert_splice_equals_ref(notes, ptr, 5, [(0, 0, 2, 1), (0, 1, 0, 1)], [0, 2], 3)
    assert want[4][:2] == [1, 0]
    # seg_ptr: negative, beyond S, decreasing; clamped, never followed
    segments = [(0, 0, 0, 2), (1, 1, 0, 2), (0, 3, 0, 2)]
    for seg_ptr, n_bad in (([-4, 1, 2, 3], 1), ([0, 1, 7, 3], 2), ([0, 2, 1, 3], 1), ([0, 1, 2, 1 << 30], 1), ([5, 0, -1, 2], 3)):
        want = assert_splice_equals_ref(notes, ptr, 5, segments, seg_ptr, 2, rule=1)
        assert want[4][1] == n_bad
        nb = batch_of(unsorted_songs(), 5)
        with pytest.raises(ValueError, match=f"seg_ptr: {n_bad} bad entries"):
            ops.notes_splice(nb.notes, nb.track_ptr, 5, dev(np.asarray(segments, np.int32)), dev(np.asarray(seg_ptr, np.int32)), 2)
    # a track_ptr that breaks the contract is clamped, as in the statistics
    bad = ptr.copy()
    bad[2], bad[5], bad[7] = -4, len(notes) + 9, 1
    assert_splice_equals_ref(notes, bad, 5, segments, [0, 1, 2, 3], 2, shift=[1, 2, 3])


def test_a_capacity_below_the_need():
    notes, ptr = flat(unsorted_songs())
    segments, seg_ptr = [(0, 0, 0, 2), (0, 1, 0, 2), (1, 0, 0, 2), (1, 1, 0, 2)], [0, 1, 2, 3, 4]
    need = splice_ref(notes, ptr, 5, segments, seg_ptr, 2)[2][0]
    assert need > 64
    for cap in (need - 5, need, need + 5, 1, 0):
        want = assert_splice_equals_ref(notes, ptr, 5, segments, seg_ptr, 2, shift=[0, 1, 2, 3], cap=cap)
        assert want[2][0] == need and want[4][2] == max(need - cap, 0)
    nb = batch_of(unsorted_songs(), 5)
    args = (nb.notes, nb.track_ptr, 5, dev(np.asarray(segments, np.int32)), dev(np.asarray(seg_ptr, np.int32)), 2)
    with pytest.raises(ValueError, match="5 rows beyond the capacity"):
        ops.notes_splice(*args, capacity=need - 5)
    out, _, totals, _, status = ops.notes_splice(*args, capacity=need - 5, check=False)
    assert out.shape == (need - 5, 3) and totals[0].item() == need and status.tolist() == [0, 0, 5, 0]
    assert ops.notes_splice(*args)[0].shape == nb.notes.shape                              # the default: the input's rows


# ---- the reference's silence filter -----------------------------------------------------------------------------------------------
def from_acts(acts):
    """a piece with one note in every active (track, bar)"""
    return [[(32 * b + 3 * k, 60 + k, 4) for b, on in enumerate(row) if on] for k, row in enumerate(acts)]


GRIDS = {"two consecutive silent bars": [[1, 1], [1, 1], [0, 0], [1, 1]], "a bar silent in every track": [[1, 0], [1, 0], [1, 0], [1, 0]],
         "cross-track": [[0, 1], [1, 0], [1, 1], [1, 1]], "full": [[1, 1], [1, 1], [1, 1], [1, 1]],
         "silent bars 1 then 0": [[1, 0], [1, 1], [1, 1], [0, 1]], "one silent bar": [[1, 1], [1, 1], [1, 1], [1, 0]]}


def test_filter_keeps_what_the_reference_keeps():
    pieces = [from_acts(g) for g in GRIDS.values()]
    want_keep = [filter_ref(np.asarray(g, bool)) for g in GRIDS.values()]
    assert want_keep == [False, False, False, True, True, True]
    nb = NoteBatch.from_lists(pieces, 2, device=DEV)
    got, index = nb.windows(2, filter="reference")
    assert lists(got) == [p for p, k in zip(pieces, want_keep) if k] and index.song.tolist() == [3, 4, 5] and index.start.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="rejects all 3 windows"):
        nb.select([0, 1, 2]).windows(2, filter="reference")
    # sliding over drawn songs: W = 3 and W = 2 with both strides, W = 1
    rng = np.random.default_rng(3)
    drawn = ([from_acts(rng.random((4, 7)) < 0.8) for _ in range(6)]
             + [from_acts(np.zeros((4, 7), bool)), from_acts(np.eye(4, 7, dtype=bool)), from_acts(np.ones((4, 7), bool))])
    nb = NoteBatch.from_lists(drawn, 7, device=DEV)
    seen = set()
    for W, stride in ((3, 1), (2, 1), (2, 2), (1, 1), (7, 1)):
        every, song, start = windows_np(drawn, W, stride, total_bars=7)
        keep = [filter_ref(window_acts(w, W)) for w in every]
        seen |= set(keep)
        got, index = nb.windows(W, stride=stride, filter="reference", transpose=2)
        kept = [i for i, k in enumerate(keep) if k]
        assert lists(got) == [transposed(every[i], 2) for i in kept] and got.n_bars == W
        assert index.song.tolist() == [song[i] for i in kept] and index.start.tolist() == [start[i] for i in kept]
        assert index.shift.tolist() == [2] * len(kept) and got.track_ptr.shape == (4 * len(kept) + 1,)
        notes, ptr = flat(drawn)
        want = assert_splice_equals_ref(notes, ptr, 7, [(b, s, 0, W) for b, s in zip(song, start)], list(range(len(every) + 1)), W, rule=1)
        assert want[3] == [int(k) for k in keep]
    assert seen == {True, False}


def test_filter_at_its_longest_window():
    """64 bars: every bit of the mask; bar 63 silent in one track, then bars 62 and 63 in it, then bar 63 in all"""
    acts = np.ones((4, 64), bool)
    acts[2, 63] = acts[0, 31] = acts[1, 33] = False
    two = acts.copy()
    two[2, 62] = False
    cross = acts.copy()
    cross[3, 0] = False                                            # 63 of track 2, then 0 of track 3: -63
    cross1 = acts.copy()
    cross1[1, 32], cross1[1, 33] = False, True                     # 31 of track 0, then 32 of track 1
    column = acts.copy()
    column[:, 63] = False
    grids = [acts, two, cross, cross1, column]
    want_keep = [filter_ref(g) for g in grids]
    assert want_keep == [True, False, True, False, False]
    pieces = [from_acts(g) for g in grids]
    nb = NoteBatch.from_lists(pieces, 64, device=DEV)
    got, index = nb.windows(64, filter="reference")
    assert index.song.tolist() == [0, 2] and lists(got) == [pieces[0], pieces[2]]
    long = NoteBatch.from_lists([from_acts(np.ones((4, 66), bool))], 66, device=DEV)
    with pytest.raises(ValueError, match="n_bars <= 64"):
        long.windows(65, filter="reference")
    got, _ = long.windows(65)                                      # without the rule there is no limit
    assert got.n_bars == 65 and lists(got) == windows_np(lists(long), 65, 1, total_bars=66)[0]
    with pytest.raises(ValueError, match="out_bars <= 64"):
        ops.notes_splice(long.notes, long.track_ptr, 66, dev(np.asarray([[0, 0, 0, 65]], np.int32)), dev(np.asarray([0, 1], np.int32)), 65,
                         silence_rule=True)


# ---- transposition ----------------------------------------------------------------------------------------------------------------
def test_transpose():
    pieces = songs(seed=4)
    pieces[0][0] += [(159, 200, 1), (159, -3, 1)]                  # drums: never touched, not even clamped
    pieces[0][1] += [(159, 200, 1), (159, -3, 1), (159, 125, 1), (159, 3, 1)]
    pieces[1][3] += [(159, 127, 1), (159, 0, 1)]
    nb = NoteBatch.from_lists(pieces, 5, device=DEV)
    every, _, _ = windows_np(pieces, 2, 1, total_bars=5)
    K = len(every)
    assert K == 8
    plain, index = nb.windows(2)
    assert lists(plain) == every and index.shift.tolist() == [0] * K                        # no shift: pitches as they are
    assert (200 in [r[1] for r in lists(plain)[3][1]]) and (-3 in [r[1] for r in lists(plain)[3][1]])
    for shift in (0, 3, -5, 6, 127, -127):
        got, index = nb.windows(2, transpose=shift)
        assert lists(got) == [transposed(w, shift) for w in every] and index.shift.tolist() == [shift] * K
        assert [t[0] for t in lists(got)] == [w[0] for w in every]                          # the drums
    per_window = [-5, 6, 0, 100, -100, 1, -1, 2]
    for t in (torch.tensor(per_window, device=DEV), torch.tensor(per_window, dtype=torch.int32, device=DEV)):
        got, index = nb.windows(2, transpose=t)
        assert lists(got) == [transposed(w, s) for w, s in zip(every, per_window)] and index.shift.tolist() == per_window
    a, ia = nb.windows(2, transpose="random", seed=7)
    b, ib = nb.windows(2, transpose="random", seed=7)
    shifts = ia.shift.tolist()
    assert ia.shift.dtype == torch.int32 and shifts == ib.shift.tolist() and all(-5 <= s <= 6 for s in shifts) and len(set(shifts)) > 1
    assert lists(a) == lists(b) == [transposed(w, s) for w, s in zip(every, shifts)]
    many = torch.cat([nb.windows(2, transpose="random", seed=s)[1].shift for s in range(40)]).tolist()
    assert set(many) == set(range(-5, 7))                          # 320 draws of 12 values
    assert nb.windows(2, transpose="random", seed=8)[1].shift.tolist() != shifts
    torch.manual_seed(5)
    free = nb.windows(2, transpose="random")[1].shift.tolist()
    assert all(-5 <= s <= 6 for s in free)
    # with the filter the shifts are those of the windows that stay
    bars, per_bar = windows_np(pieces, 1, 1, total_bars=5)[0], list(range(-5, 5))
    got, index = nb.windows(1, filter="reference", transpose=torch.tensor(per_bar, device=DEV))
    keep = [filter_ref(window_acts(w, 1)) for w in bars]
    assert any(keep) and index.shift.tolist() == [s for s, k in zip(per_bar, keep) if k]
    assert lists(got) == [transposed(w, s) for w, s, k in zip(bars, per_bar, keep) if k]


# ---- round trips on the recorded reference pieces ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    """(the 8 recorded pieces of 2 bars as a NoteBatch, as lists)"""
    notes, ptr = load_notes("lmd2_tiny")
    nb = NoteBatch(dev(notes), dev(ptr), dev(np.asarray([len(notes), 0], np.int32)), 2)
    return nb, as_lists(notes, ptr)


PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7]]


def test_join_and_round_trips(recorded):
    nb, pieces = recorded
    song = nb.join(PAIRS)
    assert isinstance(song, NoteBatch) and song.n_bars == 4 and song.resolution == nb.resolution and song.notes.shape == nb.notes.shape
    want = join_np(pieces, PAIRS, 2)
    assert lists(song) == want and sum(len(t) for p in want for t in p) == len(nb.notes) == song.totals[0].item()
    for index in (torch.tensor(PAIRS, device=DEV), torch.tensor(PAIRS, dtype=torch.int32, device=DEV), [tuple(r) for r in PAIRS]):
        assert lists(nb.join(index)) == want
    # windows of a joined song are the pieces; joined again they are the song
    wins, index = song.windows(2, stride=2)
    assert lists(wins) == pieces and index.song.tolist() == [0, 0, 1, 1, 2, 2, 3, 3] and index.start.tolist() == [0, 2] * 4
    assert lists(wins.join(PAIRS)) == want
    # ... and so are the overlapping windows, each giving its first bar, the last one both
    wins, index = song.windows(2, stride=1)
    assert lists(wins) == windows_np(want, 2, 1, total_bars=4)[0]
    triples = [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    assert lists(wins.join(triples, hop_bars=1)) == want and wins.join(triples, hop_bars=1).n_bars == 4
    assert lists(song.windows(1)[0].join(torch.arange(16, device=DEV).view(4, 4))) == want
    # any order, silent windows, one window, hop below W
    index = [[7, -1, 0], [-1, -1, 3]]
    got = nb.join(index)
    assert got.n_bars == 6 and lists(got) == join_np(pieces, index, 2)
    assert lists(got)[1] == [[(t + 128, p, d) for (t, p, d) in track] for track in pieces[3]]
    got = nb.join([[5, 2, -1, 6]], hop_bars=1)
    assert got.n_bars == 5 and lists(got) == join_np(pieces, [[5, 2, -1, 6]], 2, hop=1)
    assert lists(nb.join([[4]])) == [pieces[4]] and lists(nb.join([[-1]])) == [[[], [], [], []]]
    # entries that are neither a piece nor -1, and pieces taken twice
    for index, what in (([[0, 8]], "1 entries outside"), ([[-2, 1]], "1 entries outside"), ([[0, 1], [1, 0]], "2 entries that repeat"),
                        (torch.tensor([[1 << 40, 0, 0]], device=DEV), "1 entries outside .* 1 entries that repeat")):
        with pytest.raises(ValueError, match=what):
            nb.join(index)
    assert lists(nb.join([[0, 8], [-2, 1]], check=False)) == join_np(pieces, [[0, -1], [-1, 1]], 2)


def test_cutting_and_joining_read_nothing_back(recorded):
    """with device tensors in and `check` off neither `windows` nor `join` synchronises: what `vary_song` adds to the host reads
    of `vary_notes` is nothing"""
    nb, pieces = recorded
    index = torch.tensor(PAIRS, device=DEV)
    bars = torch.tensor([4, 4, 2, 3], device=DEV)
    shifts = torch.zeros(8, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        song = nb.join(index, check=False)
        wins, _ = song.windows(2, stride=2, check=False)
        also, _ = song.windows(2, stride=2, song_bars=bars, transpose=shifts, check=False)
        rand, _ = song.windows(2, stride=2, transpose="random", seed=3, check=False)
        again = wins.join(index, hop_bars=2, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert lists(again) == lists(song) == join_np(pieces, PAIRS, 2) and lists(wins) == pieces
    assert lists(also)[:5] == [[[(t, min(max(p, 0), 127) if k else p, d) for (t, p, d) in track] for k, track in enumerate(w)] for w in pieces[:5]]


# ---- the golden model -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    z, cfg = load_case("lmd2_tiny")
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    assert cfg["n_bars"] == 2
    return vae


def test_encode_song_is_encode_notes_on_the_host_cut_windows(model, recorded):
    nb, pieces = recorded
    song = nb.join(PAIRS)
    cut = NoteBatch.from_lists(windows_np(lists(song), 2, 2, total_bars=4)[0], 2, device=DEV)
    mu, log_var = encode_song(model, song)
    want_mu, want_lv = encode_notes(model, cut)
    assert mu.shape == log_var.shape == (4, 2, want_mu.shape[1]) and mu.dtype == torch.float32
    assert torch.equal(mu.view(8, -1), want_mu) and torch.equal(log_var.view(8, -1), want_lv)
    assert not model.training
    # a song of 3 bars is a song of 4 with a silent last bar; one of a single window
    three = NoteBatch.from_lists([[[r for r in track if r[0] < 96] for track in p] for p in lists(song)], 3, device=DEV)
    cut3 = NoteBatch.from_lists(windows_np(lists(three), 2, 2, total_bars=4)[0], 2, device=DEV)
    mu3, lv3 = encode_song(model, three)
    assert mu3.shape == (4, 2, want_mu.shape[1]) and torch.equal(mu3.view(8, -1), encode_notes(model, cut3)[0])
    assert torch.equal(lv3.view(8, -1), encode_notes(model, cut3)[1])
    mu1, _ = encode_song(model, nb)
    assert mu1.shape == (8, 1, want_mu.shape[1]) and torch.equal(mu1[:, 0], want_mu)
    with pytest.raises(ValueError, match="song must be a NoteBatch"):
        encode_song(model, lists(song))


def test_vary_song_is_vary_notes_on_the_windows_joined_on_the_host(model, recorded):
    nb, pieces = recorded
    song = nb.join(PAIRS)
    cut = NoteBatch.from_lists(windows_np(lists(song), 2, 2, total_bars=4)[0], 2, device=DEV)
    for kw in (dict(strength=0, seed=5), dict(strength=0.5, seed=6, temperature=0.9), dict(keep_structure=True, seed=7)):
        with torch.no_grad():
            got = vary_song(model, song, **kw)
            want = vary_notes(model, cut, **kw)[0]
        assert isinstance(got, NoteBatch) and got.n_bars == 4 and got.notes.is_cuda
        assert lists(got) == join_np(lists(want), PAIRS, 2) and got.totals[0].item() == want.totals[0].item()
    # 3 bars in, 4 bars out
    three = NoteBatch.from_lists([[[r for r in track if r[0] < 96] for track in p] for p in lists(song)], 3, device=DEV)
    cut3 = NoteBatch.from_lists(windows_np(lists(three), 2, 2, total_bars=4)[0], 2, device=DEV)
    with torch.no_grad():
        got = vary_song(model, three, strength=0, seed=5)
        want = vary_notes(model, cut3, strength=0, seed=5)[0]
    assert got.n_bars == 4 and lists(got) == join_np(lists(want), PAIRS, 2)


def test_a_song_with_a_wholly_silent_window(model, recorded):
    nb, pieces = recorded
    song = nb.join([[0, -1, 1]])                                   # bars 2-3 hold nothing
    wins, _ = song.windows(2, stride=2)
    assert lists(wins) == [pieces[0], [[], [], [], []], pieces[1]]
    graph = wins.to_graph()
    s = graph.s_tensor.view(3, 2, 4, 32)
    assert s[1].sum().item() == 2 and s[1, 0, 0, 0].item() == 1 and s[1, 1, 0, 0].item() == 1      # cell [0,0] of an empty bar
    mu, _ = encode_song(model, song)
    silent = NoteBatch.from_lists([[[], [], [], []]], 2, device=DEV)
    both = NoteBatch.from_lists([pieces[0], [[], [], [], []], pieces[1]], 2, device=DEV)
    assert mu.shape[:2] == (1, 3) and torch.equal(mu[0], encode_notes(model, both)[0])
    assert encode_notes(model, silent)[0].shape == (1, mu.shape[2])
    with torch.no_grad():
        got = vary_song(model, song, strength=0, seed=2)
        want = vary_notes(model, both, strength=0, seed=2)[0]
    assert got.n_bars == 6 and lists(got) == join_np(lists(want), [[0, 1, 2]], 2)
