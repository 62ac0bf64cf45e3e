"""Chord-aware sampling on the device (k_sample_chords of csrc/sample.hip, k_node_tracks of csrc/generate.hip,
`generate_music(chord_rules=...)`) against an fp64 numpy restatement of the definition in include/polyphemus_hip.h
("Chord-aware sampling"), the invariants of a chord, `pm_sample_tokens` on the same noise, the binomial bounds of the
distribution it must draw from, and a numpy restatement of the slot loop of the reference's `muspy_from_mtp`."""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import ChordRules, generate_music, pitch_mask
from polyphemus_amd.model import VAE
from test_sampling_abi import sample_hash_np
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF = None
EOS_P, PAD_P, EOS_D, PAD_D = 129, 130, 97, 98
CONFIGS = [(1.0, 1.0, OFF, OFF), (0.5, 1.5, 5, OFF), (1.5, 0.7, OFF, 0.9), (1.0, 1.0, 40, 0.9)]   # (T_pitch, T_dur, top_k, top_p)
SCORE_GAP, MASS_EDGE, LEFT_OUT_CAP = 1e-3, 1e-5, 0.05
MAX_NOTES, MIN_NOTES = (14, 1, 6, 14), (1, 1, 2, 0)
ALLOWED = np.stack([pitch_mask(), pitch_mask(28, 60), pitch_mask(40, 88, (0, 2, 4, 5, 7, 9, 11)), pitch_mask(60, 62)])
RULES = dict(min_notes=MIN_NOTES, max_notes=MAX_NOTES, allowed_pitches=ALLOWED)
SIZES, SCALES = (1, 5, 273), (1, 3)


def tracks_of(N):
    return (np.arange(N) * 7 // 3) % 4


def make_logits(N, scale):
    x = torch.randn(N, 15, 230, generator=torch.Generator().manual_seed(5000 + 100 * N + scale)) * scale
    x[:, :, EOS_P] += 2 * scale                     # without the raise nearly every chord runs to max_notes
    return x


def _draw(l, cand, head, rows, T, top_k, top_p, seed):
    """One head of one slot of every node at once: the definition of pm_sample_tokens restricted to the candidates, in fp64 on
    the fp32 logits l [N,V] (cand [N,V] bool, at least one per row): (token [N], decided [N]).  A draw is not decided when its
    two best scores are closer than SCORE_GAP or some candidate's outranking mass is within MASS_EDGE * Z of the nucleus edge."""
    N, V = l.shape
    decided = np.ones(N, bool)
    lm = np.where(cand, l, -np.inf)
    order = np.argsort(-lm, axis=1, kind="stable")                              # equal logits: lower index first; absent columns last
    if T == 0:
        return order[:, 0], decided
    inv_t = float(np.float32(1.0 / T))
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(V), order.shape), axis=1)
    live = cand & (rank < top_k) if top_k is not None else cand.copy()
    if top_p is not None and top_p < 1:
        q = np.where(live, np.exp((l - lm.max(1, keepdims=True)) * inv_t), 0.0)
        qs = np.take_along_axis(q, order, axis=1)
        before = np.empty_like(q)
        np.put_along_axis(before, order, np.cumsum(qs, axis=1) - qs, axis=1)    # mass of the survivors that outrank it
        Z = q.sum(1, keepdims=True)
        edge = float(np.float32(top_p)) * Z
        decided &= ~(live & (np.abs(before - edge) < MASS_EDGE * Z)).any(1)
        live &= before < edge
    u = (sample_hash_np(seed, rows.astype(np.uint64)[:, None], head, np.arange(V, dtype=np.uint64)[None, :]).astype(np.float64) + 0.5) / (1 << 23)
    score = np.where(live, l * inv_t - np.log(-np.log(u)), -np.inf)
    tok = score.argmax(1)                                                       # numpy: the first of equal maxima
    top2 = np.sort(score, axis=1)[:, -2:]
    decided &= ~(top2[:, 1] - top2[:, 0] < SCORE_GAP)
    return tok, decided


def pitch_candidates(count, used, track, min_notes, max_notes, allowed):
    """[N,131] bool from the chord state: count [N], used [N,128] bool, track [N]."""
    N = count.shape[0]
    cand = np.zeros((N, 131), bool)
    cand[:, :128] = allowed[track] & ~used & (count < np.asarray(max_notes)[track])[:, None]
    cand[:, EOS_P] = (count >= np.asarray(min_notes)[track]) | ~cand[:, :128].any(1)
    return cand


def replica(logits, track, T_pitch, T_dur, top_k, top_p, seed, min_notes, max_notes, allowed):
    """The definition in fp64 on the fp32 logits [N,15,230], every chord slot by slot (all the nodes' chords side by side):
    (tokens [N,15,2], note_count [N], decided [N]).  A node is decided only if every draw of its chord is."""
    N = logits.shape[0]
    l = logits.astype(np.float64)
    tokens = np.empty((N, 15, 2), np.int64)
    tokens[..., 0], tokens[..., 1] = PAD_P, PAD_D
    count, used, ended, decided = np.zeros(N, np.int64), np.zeros((N, 128), bool), np.zeros(N, bool), np.ones(N, bool)
    dur_cand = np.zeros((N, 99), bool)
    dur_cand[:, :96] = True
    for s in range(15):
        act = np.flatnonzero(~ended)
        if act.size == 0:
            break
        rows = act * 15 + s
        cand = pitch_candidates(count[act], used[act], track[act], min_notes, max_notes, allowed)
        p, dp = _draw(l[act, s, :131], cand, 0, rows, T_pitch, top_k, top_p, seed)
        assert cand[np.arange(act.size), p].all()
        eos = p == EOS_P
        d, dd = _draw(l[act, s, 131:], dur_cand[act], 1, rows, T_dur, top_k, top_p, seed)
        decided[act] &= dp & (dd | eos)
        tokens[act, s, 0] = p
        tokens[act, s, 1] = np.where(eos, EOS_D, d)
        note = act[~eos]
        used[note, p[~eos]] = True
        count[note] += 1
        ended[act[eos]] = True
    assert ended.all()
    return tokens, count, decided


_CASES = {}


def case(N, scale, i):
    """(logits, track, device tokens, device counts, replica tokens, replica counts, decided) of one case, computed once."""
    key = (N, scale, i)
    if key not in _CASES:
        Tp, Td, k, p = CONFIGS[i]
        logits, track = make_logits(N, scale), tracks_of(N)
        tok, cnt = ops.sample_chords(logits.to(DEV), torch.from_numpy(track.astype(np.uint8)).to(DEV), (Tp, Td), k, p, 1000 + i, **RULES)
        assert tok.shape == (N, 15, 2) and tok.dtype == torch.int32 and cnt.shape == (N,) and cnt.dtype == torch.int32
        want = replica(logits.numpy(), track, Tp, Td, k, p, 1000 + i, MIN_NOTES, MAX_NOTES, ALLOWED)
        _CASES[key] = (logits, track, tok.cpu().numpy(), cnt.cpu().numpy()) + want
    return _CASES[key]


@pytest.mark.parametrize("N", SIZES)
def test_chords_equal_the_fp64_replica(N):
    """A case is one (N, scale, configuration).  At exactly these inputs the replica alone (nothing of the device enters that)
    leaves out no node at N = 1 and N = 5 and at most 0.0293 of the nodes at N = 273; the cap is 0.05."""
    hist = np.zeros(15, np.int64)
    for scale in SCALES:
        for i in range(len(CONFIGS)):
            _, _, got, got_n, want, want_n, decided = case(N, scale, i)
            left_out = 1.0 - decided.mean()
            differ = int(((got != want).any((1, 2)) | (got_n != want_n))[decided].sum())
            print(f"N={N} scale={scale} config={CONFIGS[i]}: {left_out:.4f} of the nodes left out, {differ} decided nodes differ")
            assert left_out <= LEFT_OUT_CAP, (N, scale, i, left_out)
            assert np.array_equal(got[decided], want[decided]), (N, scale, i, np.flatnonzero((got != want).any((1, 2)) & decided)[:8])
            assert np.array_equal(got_n[decided], want_n[decided]), (N, scale, i)
            hist += np.bincount(want_n, minlength=15)
    if N == 273:
        print("note counts of the replica over the eight cases:", hist.tolist())
        assert (hist > 0).all(), hist                      # the test keeps exercising chords of every length 0..14


def check_invariants(tokens, note_count, track, min_notes=MIN_NOTES, max_notes=MAX_NOTES, allowed=ALLOWED):
    """tokens [N,15,2] are `count` note pairs, then (EOS, EOS), then (PAD, PAD); the pitches distinct and allowed; the count
    inside the track's bounds except where the mask ran out."""
    N = tokens.shape[0]
    for n in range(N):
        t, c = int(track[n]), int(note_count[n])
        tp, td = tokens[n, :, 0], tokens[n, :, 1]
        assert 0 <= c <= 14
        assert (tp[:c] >= 0).all() and (tp[:c] < 128).all() and (td[:c] >= 0).all() and (td[:c] < 96).all(), (n, tokens[n])
        assert tp[c] == EOS_P and td[c] == EOS_D, (n, tokens[n])
        assert (tp[c + 1:] == PAD_P).all() and (td[c + 1:] == PAD_D).all(), (n, tokens[n])
        assert len(set(tp[:c].tolist())) == c and allowed[t][tp[:c]].all(), (n, t, tp[:c])
        n_allowed = int(allowed[t].sum())
        if n_allowed < min_notes[t]:
            assert c == n_allowed, (n, t, c)
        else:
            assert min_notes[t] <= c <= min(max_notes[t], n_allowed), (n, t, c)


@pytest.mark.parametrize("N", SIZES)
def test_every_chord_is_notes_one_eos_then_pad_under_the_rules(N):
    seen_exhausted = False
    for scale in SCALES:
        for i in range(len(CONFIGS)):
            _, track, got, got_n, _, _, _ = case(N, scale, i)
            check_invariants(got, got_n, track)
            seen_exhausted |= bool(((track == 3) & (got_n == 3)).any())
    if N == 273:
        assert seen_exhausted                              # Strings: three allowed pitches, a mask that runs out


@pytest.mark.parametrize("T", [1.0, 0.6])
def test_chords_keep_the_tokens_of_sample_tokens_where_they_are_candidates(T):
    """Filters off: the Gumbel arg-max of the chord runs over a subset of pm_sample_tokens' columns with the same fp32 scores,
    so a free token that is a candidate is the chord's token.  Exact, no exclusions."""
    checked = np.zeros(2, np.int64)
    for N, scale in ((5, 1), (273, 1), (273, 3)):
        logits, track = make_logits(N, scale).to(DEV), tracks_of(N)
        free = ops.sample_tokens(logits, T, seed=77).cpu().numpy()
        tok, cnt = ops.sample_chords(logits, torch.from_numpy(track.astype(np.uint8)).to(DEV), (T, T), seed=77, **RULES)
        tok, cnt = tok.cpu().numpy(), cnt.cpu().numpy()
        for n in range(N):
            count, used = np.zeros(1, np.int64), np.zeros((1, 128), bool)
            for s in range(int(cnt[n]) + 1):               # the note slots and the slot of the EOS
                cand = pitch_candidates(count, used, track[n:n + 1], MIN_NOTES, MAX_NOTES, ALLOWED)[0]
                if cand[free[n, s, 0]]:
                    assert tok[n, s, 0] == free[n, s, 0], (N, scale, n, s)
                    checked[0] += 1
                if s < cnt[n]:
                    if free[n, s, 1] < 96:
                        assert tok[n, s, 1] == free[n, s, 1], (N, scale, n, s)
                        checked[1] += 1
                    used[0, tok[n, s, 0]] = True
                    count += 1
    print(f"T={T}: {checked[0]} pitch and {checked[1]} duration tokens compared")
    assert checked.min() > 500


def greedy_reference(logits, track, min_notes=MIN_NOTES, max_notes=MAX_NOTES, allowed=ALLOWED):
    """numpy arg-max over the candidates (the first of equal maxima; -0 == +0), chord by chord."""
    N = logits.shape[0]
    tokens = np.empty((N, 15, 2), np.int64)
    tokens[..., 0], tokens[..., 1] = PAD_P, PAD_D
    counts = np.zeros(N, np.int64)
    for n in range(N):
        count, used = np.zeros(1, np.int64), np.zeros((1, 128), bool)
        for s in range(15):
            cand = pitch_candidates(count, used, track[n:n + 1], min_notes, max_notes, allowed)[0]
            p = int(np.where(cand, logits[n, s, :131], -np.inf).argmax())
            if p == EOS_P:
                tokens[n, s] = (EOS_P, EOS_D)
                break
            tokens[n, s] = (p, int(logits[n, s, 131:131 + 96].argmax()))
            used[0, p] = True
            count += 1
        counts[n] = count[0]
    return tokens, counts


def test_greedy_chords_are_the_argmax_over_the_candidates():
    N = 273
    logits, track = make_logits(N, 3), tracks_of(N)
    assert track[0] == 0 and track[3] == 3 and track[4] == 1 and track[2] == 0
    logits[0, 0, 7] = logits[0, 0, 100] = 50.0                   # two equal maxima: the lower index
    logits[0, 0, 131 + 95] = logits[0, 0, 131 + 3] = 50.0
    logits[0, 1, 7] = logits[0, 1, 100] = 50.0                   # 7 is used by now: 100
    logits[0, 1, 131 + 98] = 70.0                                # the duration PAD is no candidate
    logits[2, 0, 128] = logits[2, 0, 130] = 90.0                 # neither are SOS and PAD of the pitch head
    logits[2, 1, :] = 0.25                                       # a constant row: the lowest candidate, duration 0
    logits[2, 2, :131] = -0.0
    logits[2, 2, 5] = 0.0                                        # -0 == +0: still the lowest candidate
    logits[3, 0, :] = 0.25                                       # Strings, min_notes 0: the lowest candidate is pitch 60
    logits[4, 0, 61] = 99.0                                      # Bass: 61 is outside 28..60
    want, want_n = greedy_reference(logits.numpy(), track)
    assert tuple(want[0, 0]) == (7, 3) and want[0, 1, 0] == 100 and want[0, 1, 1] < 96 and want[2, 0, 0] < 128
    assert tuple(want[2, 1]) == (0, 0) and want[2, 2, 0] == 1 and tuple(want[3, 0]) == (60, 0) and want[4, 0, 0] != 61
    x, tr = logits.to(DEV), torch.from_numpy(track.astype(np.uint8)).to(DEV)
    greedy, greedy_n = ops.sample_chords(x, tr, 0, **RULES)
    assert np.array_equal(greedy.cpu().numpy(), want) and np.array_equal(greedy_n.cpu().numpy(), want_n)
    check_invariants(want, want_n, track)
    for kw in (dict(temperature=(0, 0), seed=5), dict(temperature=1.0, top_k=1), dict(temperature=(0.3, 2.0), top_k=1, seed=9),
               dict(temperature=5.0, top_k=1, top_p=0.5), dict(temperature=0, top_k=7, top_p=0.4, seed=3)):
        tok, cnt = ops.sample_chords(x, tr, **kw, **RULES)
        assert torch.equal(tok, greedy) and torch.equal(cnt, greedy_n), kw
    # greedy pitches, sampled durations: the chords' pitches and ends are those of (0, 0), the durations are drawn
    for kw in (dict(), dict(top_k=40), dict(top_p=0.9)):
        tok, cnt = ops.sample_chords(x, tr, (0, 1), seed=4, **kw, **RULES)
        assert torch.equal(tok[..., 0], greedy[..., 0]) and torch.equal(cnt, greedy_n), kw
        assert not torch.equal(tok[..., 1], greedy[..., 1])
        check_invariants(tok.cpu().numpy(), cnt.cpu().numpy(), track)
    tok, cnt = ops.sample_chords(x, tr, (1, 0), seed=4, **RULES)  # and the other way round: arg-max durations on drawn chords
    tok = tok.cpu().numpy()
    notes = tok[..., 0] < 128
    assert np.array_equal(tok[..., 1][notes], logits.numpy()[..., 131:131 + 96].argmax(-1)[notes])
    assert not np.array_equal(tok[..., 0], want[..., 0])


# ---- the distribution: N identical nodes on one track, a known law per head -------------------------------------------
N_DIST, TRACK_DIST, MASKED = 16384, 2, 45
P_PITCH = {40: 0.35, 43: 0.25, MASKED: 0.2, 47: 0.1, EOS_P: 0.1}      # 45 carries mass and is masked out: four candidates remain
P_DUR = {0: 0.4, 63: 0.3, 64: 0.2, 98: 0.1}                           # 98 (PAD) is no candidate


@pytest.fixture(scope="module")
def dist():
    row = torch.full((230,), -30.0)
    for t, p in P_PITCH.items():
        row[t] = float(np.log(p))
    for t, p in P_DUR.items():
        row[131 + t] = float(np.log(p))
    allowed = np.ones((4, 128), bool)
    allowed[TRACK_DIST, MASKED] = False
    return (row.expand(N_DIST, 15, 230).contiguous().to(DEV), torch.full((N_DIST,), TRACK_DIST, dtype=torch.uint8, device=DEV), allowed)


def _law(p, without=()):
    """the law renormalised over the candidates (the columns at -30 hold 1e-11 of the mass: far inside every bound)"""
    keep = {t: v for t, v in p.items() if t not in without}
    z = sum(keep.values())
    return {t: v / z for t, v in keep.items()}


def _check(tokens, law, R, what, only=True):
    """the share of every token of the law among `tokens` [R] within 5 sigma of the binomial, and (`only`) no other token drawn"""
    assert tokens.shape == (R,) and R > 0
    for t, e in law.items():
        g = float((tokens == t).mean())
        bound = 5.0 * (e * (1.0 - e) / R) ** 0.5
        print(f"{what} token {t}: share {g:.5f}, expected {e:.5f} +- {bound:.5f} (R = {R})")
        assert abs(g - e) <= bound, (what, t, g, e, bound)
    assert not only or np.isin(tokens, list(law)).all(), (what, np.setdiff1d(tokens, list(law)))


def test_chord_shares_follow_the_renormalised_laws(dist):
    x, tr, allowed = dist
    pitches = (40, 43, 47)
    # min_notes = 0: slot 0 over {40, 43, 47, EOS}; slot 1, given the pitch of slot 0, over the law without that pitch
    tok, cnt = ops.sample_chords(x, tr, seed=11, min_notes=0, max_notes=14, allowed_pitches=allowed)
    t0 = tok.cpu().numpy()
    check_invariants(t0, cnt.cpu().numpy(), np.full(N_DIST, TRACK_DIST), (0,) * 4, (14,) * 4, allowed)
    _check(t0[:, 0, 0], _law(P_PITCH, (MASKED,)), N_DIST, "min_notes=0 slot 0")
    for a in pitches:
        sel = t0[:, 0, 0] == a
        _check(t0[sel, 1, 0], _law(P_PITCH, (MASKED, a)), int(sel.sum()), f"min_notes=0 slot 1 after {a}")
    sel = t0[:, 0, 0] == EOS_P
    assert (t0[sel, 1, 0] == PAD_P).all() and (t0[sel, 0, 1] == EOS_D).all()
    # min_notes = 1: slot 0 never gives the EOS and renormalises without it; slot 1 is as above
    tok1, cnt1 = ops.sample_chords(x, tr, seed=12, min_notes=1, max_notes=14, allowed_pitches=allowed)
    t1 = tok1.cpu().numpy()
    assert (t1[:, 0, 0] != EOS_P).all() and int(cnt1.min()) >= 1
    _check(t1[:, 0, 0], _law(P_PITCH, (MASKED, EOS_P)), N_DIST, "min_notes=1 slot 0")
    for a in pitches:
        sel = t1[:, 0, 0] == a
        _check(t1[sel, 1, 0], _law(P_PITCH, (MASKED, a)), int(sel.sum()), f"min_notes=1 slot 1 after {a}")
    # a temperature per head: the pitch law at T = 2 is proportional to sqrt(p), the duration law at T = 1 stays
    tok2, _ = ops.sample_chords(x, tr, (2.0, 1.0), seed=13, min_notes=1, max_notes=14, allowed_pitches=allowed)
    t2 = tok2.cpu().numpy()
    # (at T = 2 the 124 candidates at -30 together hold 3e-5 of the mass: far inside the bounds, but one may be drawn)
    _check(t2[:, 0, 0], _law({t: p ** 0.5 for t, p in P_PITCH.items()}, (MASKED, EOS_P)), N_DIST, "T=(2,1) slot 0", only=False)
    # durations: the law renormalised over 0..95, independent of the pitch
    law_d, law_p = _law(P_DUR, (98,)), _law(P_PITCH, (MASKED, EOS_P))
    for t in (t1, t2):
        _check(t[:, 0, 1], law_d, N_DIST, "duration of slot 0")
    for a, pa in law_p.items():
        for d, pd in law_d.items():
            joint = float(((t1[:, 0, 0] == a) & (t1[:, 0, 1] == d)).mean())
            assert abs(joint - pa * pd) <= 5.0 * (pa * pd * (1 - pa * pd) / N_DIST) ** 0.5, (a, d, joint, pa * pd)
    # seeds: two differ, one repeats bit for bit
    again, again_n = ops.sample_chords(x, tr, seed=12, min_notes=1, max_notes=14, allowed_pitches=allowed)
    assert torch.equal(again, tok1) and torch.equal(again_n, cnt1)
    other, _ = ops.sample_chords(x, tr, seed=14, min_notes=1, max_notes=14, allowed_pitches=allowed)
    same = float((other.cpu().numpy()[:, 0, 0] == t1[:, 0, 0]).mean())
    p2 = sum(p * p for p in law_p.values())                        # two seeds agree on a row with probability sum p^2
    assert abs(same - p2) <= 5.0 * (p2 * (1 - p2) / N_DIST) ** 0.5, (same, p2)


def test_non_finite_logits_give_chords_in_range_and_touch_nothing_else():
    N, pad, canary = 3, 5, -123456789
    logits = torch.randn(N, 15, 230, generator=torch.Generator().manual_seed(2))
    logits[:, :, EOS_P] -= 4.0                                    # chords that run on, so that the patterned rows are reached
    logits[0, 0, 5] = float("nan")
    logits[0, 1, 140] = float("nan")
    logits[0, 2] = float("nan")
    logits[0, 3, 7] = float("inf")
    logits[0, 3, 9] = float("inf")
    logits[0, 4, 131:] = float("inf")
    logits[0, 5, 20] = -float("inf")
    logits[0, 6] = -float("inf")
    logits[0, 7, :131] = -float("inf")
    logits[0, 8, ::2] = float("inf")
    logits[0, 8, 1::2] = -float("inf")
    logits[0, 9, 0] = float("nan")
    logits[0, 9, 1] = float("inf")
    logits[0, 9, 2] = -float("inf")
    logits[0, 10] = 3.0e38
    logits[0, 11] = -3.0e38
    logits[1] = logits[0]                                         # the same rows under the Guitar's and the Strings' rules
    logits[2, :8] = logits[0, 2:10]
    x = logits.to(DEV)
    tr = torch.tensor([0, 2, 3], dtype=torch.uint8, device=DEV)
    mask = ops.check_chord_args(allowed_pitches=ALLOWED)[3]
    for kw in (dict(temperature=(0.0, 0.0)), dict(temperature=(1.0, 1.0)), dict(temperature=(1e-30, 1e30)), dict(temperature=(0.0, 1.0)),
               dict(temperature=(1.0, 0.0), top_k=5), dict(temperature=(0.5, 0.5), top_k=5), dict(temperature=(1.5, 1.5), top_p=0.9),
               dict(temperature=(1.0, 1.0), top_k=40, top_p=0.9)):
        rules = _lib.PmChordRules()
        rules.temperature[0], rules.temperature[1] = kw["temperature"]
        rules.top_k, rules.top_p = kw.get("top_k", 0), kw.get("top_p", 1.0)
        for k in range(4):
            rules.min_notes[k], rules.max_notes[k] = MIN_NOTES[k], MAX_NOTES[k]
            for w in range(4):
                rules.pitch_mask[k][w] = mask[k][w]
        buf = torch.full((pad + N * 30 + pad,), canary, dtype=torch.int32, device=DEV)
        cbuf = torch.full((pad + N + pad,), canary, dtype=torch.int32, device=DEV)
        _lib.call("pm_sample_chords", x.data_ptr(), tr.data_ptr(), N, ctypes.addressof(rules), 21, buf.data_ptr() + 4 * pad,
                  cbuf.data_ptr() + 4 * pad, _lib.stream())
        out, cout = buf.cpu().numpy(), cbuf.cpu().numpy()
        assert (out[:pad] == canary).all() and (out[-pad:] == canary).all() and (cout[:pad] == canary).all() and (cout[-pad:] == canary).all(), kw
        tok, cnt = out[pad:-pad].reshape(N, 15, 2), cout[pad:-pad]
        assert tok.min() >= 0 and (tok[..., 0] < 131).all() and (tok[..., 1] < 99).all(), kw
        assert cnt.min() >= 0 and cnt.max() <= 14, kw
        buf2 = torch.full((pad + N * 30 + pad,), canary, dtype=torch.int32, device=DEV)          # note_count may be NULL
        _lib.call("pm_sample_chords", x.data_ptr(), tr.data_ptr(), N, ctypes.addressof(rules), 21, buf2.data_ptr() + 4 * pad, None,
                  _lib.stream())
        assert torch.equal(buf2, buf), kw
    tok, cnt = ops.sample_chords(x[:0].contiguous(), tr[:0].contiguous())
    assert tok.shape == (0, 15, 2) and tok.dtype == torch.int32 and cnt.shape == (0,) and cnt.dtype == torch.int32


# ---- the tracks of the nodes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,p", [(1, 1.0), (5, 0.3), (64, 0.02), (33, 0.97), (1, 0.0)])
def test_node_tracks_are_the_track_indices_in_cell_order(G, p):
    s = torch.rand(1, G, 4, 32, generator=torch.Generator().manual_seed(G)) < p
    want = s.reshape(-1, 4, 32).nonzero()[:, 1].to(torch.uint8)
    N = int(s.sum())
    got = ops.node_tracks(s.to(DEV), N)
    assert got.dtype == torch.uint8 and got.shape == (N,) and torch.equal(got.cpu(), want)
    assert torch.equal(ops.node_tracks(s.float().to(DEV), N).cpu(), want)
    with pytest.raises(ValueError, match="active cells"):
        ops.node_tracks(s.to(DEV), N + 1)
    if N:
        with pytest.raises(ValueError, match="active cells"):
            ops.node_tracks(s.to(DEV), N - 1)


def test_node_tracks_zero_the_tail_and_write_nothing_behind_it():
    G, pad, canary = 5, 7, 0xA5
    s = (torch.rand(1, G, 4, 32, generator=torch.Generator().manual_seed(G)) < 0.3)
    want = s.reshape(-1, 4, 32).nonzero()[:, 1].to(torch.uint8)
    active = int(s.sum())
    sf = s.float().contiguous().to(DEV)
    for N in (active + 9, active, active - 4):
        buf = torch.full((pad + N + pad,), canary, dtype=torch.uint8, device=DEV)
        bn, npt = torch.empty(G, dtype=torch.int32, device=DEV), torch.empty(G + 1, dtype=torch.int32, device=DEV)
        _lib.call("pm_node_tracks", sf.data_ptr(), G, N, bn.data_ptr(), npt.data_ptr(), buf.data_ptr() + pad, _lib.stream())
        out = buf.cpu()
        assert (out[:pad] == canary).all() and (out[-pad:] == canary).all(), N
        assert torch.equal(out[pad:pad + min(N, active)], want[:N]) and (out[pad + active:pad + N] == 0).all(), N
        assert int(npt[G]) == active and torch.equal(bn.cpu().long(), s.reshape(G, -1).sum(1))
    got = ops.node_tracks(s.to(DEV), active + 9, check=False).cpu()
    assert torch.equal(got[:active], want) and (got[active:] == 0).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def notes_of_cells(mtp):
    """The slot loop of the reference's `muspy_from_mtp` (utils.py:99-124) over every cell of mtp [..., 15, 230]: the list of
    the pitches of the notes it reads, per cell (break on a pitch or duration EOS / PAD, skip SOS)."""
    cells = mtp.reshape(-1, 15, 230).cpu()
    pitch, dur = cells[..., :131].argmax(-1).numpy(), cells[..., 131:].argmax(-1).numpy()
    out = []
    for c in range(cells.shape[0]):
        notes = []
        for s in range(15):
            if pitch[c, s] in (EOS_P, PAD_P) or dur[c, s] in (EOS_D, PAD_D):
                break
            if pitch[c, s] == 128:
                continue
            notes.append(int(pitch[c, s]))
        out.append(notes)
    return out


E2E_RULES = ChordRules(min_notes=MIN_NOTES, max_notes=MAX_NOTES, allowed_pitches=ALLOWED)


def _check_chords(vae, z, cond, s_tensor, c_logits):
    mtp, s_out, tokens, counts = generate_music(vae, z, *cond, seed=7, chord_rules=E2E_RULES, return_tokens=True, return_note_counts=True)
    assert torch.equal(s_out, s_tensor) and mtp.shape == (*s_tensor.shape, 15, 230)
    N = c_logits.shape[0]
    track = ops.node_tracks(s_tensor, N)
    assert torch.equal(track.cpu(), s_tensor.reshape(-1, 4, 32).nonzero()[:, 1].to(torch.uint8).cpu())
    want, want_n = ops.sample_chords(c_logits, track, seed=7, **RULES)
    assert torch.equal(tokens, want) and torch.equal(counts, want_n) and counts.dtype == torch.int32 and counts.shape == (N,)
    assert torch.equal(mtp, ops.mtp_from_tokens(tokens, s_tensor))
    check_invariants(tokens.cpu().numpy(), counts.cpu().numpy(), track.cpu().numpy())
    notes = notes_of_cells(mtp)
    counts_h, track_h = counts.cpu().numpy(), track.cpu().numpy()
    active = s_tensor.reshape(-1).cpu().numpy().astype(bool)
    assert len(notes) == active.size and int(active.sum()) == N
    cell_track = (np.arange(active.size) // 32) % 4
    n = 0
    for c, ns in enumerate(notes):
        if not active[c]:
            assert ns == [], c
            continue
        assert len(ns) == int(counts_h[n]) and len(set(ns)) == len(ns) and ALLOWED[cell_track[c]][ns].all(), (c, n, ns)
        assert cell_track[c] == int(track_h[n])
        n += 1
    assert n == N
    # the shorter tuples, a temperature pair, and the constrained arg-max
    out = generate_music(vae, z, *cond, seed=7, chord_rules=E2E_RULES)
    assert len(out) == 2 and torch.equal(out[0], mtp)
    out = generate_music(vae, z, *cond, seed=7, chord_rules=E2E_RULES, return_note_counts=True)
    assert len(out) == 3 and torch.equal(out[2], counts)
    tok_g = generate_music(vae, z, *cond, temperature=(0, 0.5), seed=7, chord_rules=E2E_RULES, return_tokens=True)[2]
    assert torch.equal(tok_g, ops.sample_chords(c_logits, track, (0, 0.5), seed=7, **RULES)[0])
    return tokens


@pytest.mark.parametrize("name", ["lmd2_tiny", "nb3_tiny"])
def test_generate_music_with_chord_rules_end_to_end(name):
    z, cfg = load_case(name)
    gg = np.load(os.path.join(GOLDEN, f"{name}_generate.npz"), allow_pickle=False)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    zs = torch.from_numpy(gg["gen/z"]).to(DEV)
    with torch.no_grad():
        _, c_logits = vae.decoder(zs, None)
        c_logits = c_logits.detach().contiguous().float()
        # chord_rules=None: every path is what it is without the argument
        for kw in (dict(), dict(temperature=1, seed=7, return_tokens=True), dict(top_k=1), dict(temperature=1.0, top_p=0.95, return_tokens=True)):
            torch.manual_seed(1234)                        # seed=None takes one from torch's CPU generator
            a = generate_music(vae, zs, **kw)
            torch.manual_seed(1234)
            b = generate_music(vae, zs, chord_rules=None, **kw)
            assert len(a) == len(b) and [_sha(t) for t in a] == [_sha(t) for t in b], kw
        s0 = generate_music(vae, zs)[1]
        tokens = _check_chords(vae, zs, (), s0, c_logits)
        assert not torch.equal(tokens, generate_music(vae, zs, temperature=1, seed=7, return_tokens=True)[2])


def test_generate_music_with_chord_rules_and_structure_conditioning():
    z, cfg = load_case("lmd2_tiny")
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    s_one = torch.zeros(cfg["n_bars"], 4, 32, dtype=torch.bool)
    s_one[0, 1, ::4] = True
    s_one[0, 0, 2] = True
    s_tensor = s_one.unsqueeze(0).repeat(3, 1, 1, 1).to(DEV)
    zz = torch.randn(3, cfg["d"], generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        graph = vae.decoder._structure_from_binary(s_tensor)
        _, c_logits = vae.decoder(zz, graph)
        c_logits = c_logits.detach().contiguous().float()
        a, b = generate_music(vae, zz, graph, s_tensor), generate_music(vae, zz, graph, s_tensor, chord_rules=None)
        assert _sha(a[0]) == _sha(b[0]) and a[1] is b[1] is s_tensor
        _check_chords(vae, zz, (graph, s_tensor), s_tensor, c_logits)
