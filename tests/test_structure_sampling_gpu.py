"""Structure sampling on the device (k_sample_structure of csrc/sample.hip, `ops.sample_structure`,
`generate_music(structure_rules=...)`) against an fp64 numpy restatement of the definition in include/polyphemus_hip.h
("Structure sampling"), the invariants of a sampled bar, the thresholded rule it reduces to, the binomial bounds of the
distribution it must draw from, and end to end on the golden-case models."""
import ctypes
import math

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import ChordRules, StructureRules, generate_music, pitch_mask, step_mask
from polyphemus_amd.model import VAE
from test_sampling_abi import sample_hash_np
from util import load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 3, 515)                                  # one bar, an odd partial wave, many blocks with an odd tail
LOGITS = ((1, 0), (3, -2), (3, -8))                  # randn * scale + shift; the last leaves most thresholded bars empty
TEMPS = (0.0, 0.5, 1.0, 1.5)
MARGIN, LEFT_OUT_CAP = 1e-4, 0.05                    # fp32 evaluates a score to about 1e-6: two orders below the margin
MASKS = np.stack([step_mask(), step_mask(2), step_mask(), step_mask(8)])
RULE_SETS = (dict(),
             dict(threshold=(.5, .3, .7, .5), min_active=(2, 0, 1, 4), max_active=(8, 16, 3, 4), allowed_steps=MASKS),
             dict(max_active=(0, 2, 0, 1), allowed_steps=MASKS))


def four(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 4


def rules_of(r):
    """(bias [4] as the kernel gets it, min_active [4], max_active [4], allowed [4,32]) of a rule set"""
    bias = np.array([np.float32(math.log(t / (1.0 - t))) for t in four(r.get("threshold", 0.5))], np.float64)
    allowed = np.ones((4, 32), bool) if r.get("allowed_steps") is None else np.asarray(r["allowed_steps"])
    return bias, np.array(four(r.get("min_active", 0))), np.array(four(r.get("max_active", 32))), allowed


_BASE = {}


def make_logits(G, li):
    """the first G bars of the 515 of logit set li: the smaller calls see the same bars at the same indices"""
    if li not in _BASE:
        scale, shift = LOGITS[li]
        _BASE[li] = torch.randn(515, 4, 32, generator=torch.Generator().manual_seed(900 + li)) * scale + shift
    return _BASE[li][:G].contiguous()


def replica(x, T, seed, bias, mn, mx, allowed):
    """The definition in fp64 on the fp32 logits x [G,4,32]: (s [G,4,32] bool, counts [G,4], decided [G], empty [G] = the bars
    the no-empty-bar step filled).  A bar is not
    decided when some allowed cell has |score| < MARGIN, when the two scores on either side of a binding bound are closer than
    MARGIN (the rank min_active binds where the first cell it does not force is negative, the rank max_active where the last
    cell it admits is not), or when its empty-bar fallback has two top scores closer than MARGIN."""
    G = x.shape[0]
    score = x.astype(np.float64) - bias[None, :, None]
    if T != 0:
        g, c = np.arange(G, dtype=np.uint64)[:, None], np.arange(128, dtype=np.uint64)[None, :]
        u = ((sample_hash_np(seed, g, 2, c).astype(np.float64) + 0.5) / (1 << 23)).reshape(G, 4, 32)
        score = score * float(np.float32(1.0 / T)) + (np.log(u) - np.log1p(-u))
    al = np.broadcast_to(allowed[None], score.shape)
    keyed = np.where(al, -score, np.inf)
    order = np.argsort(keyed, axis=-1, kind="stable")                           # descending, equal scores by lower t; not allowed last
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(32), order.shape), axis=-1)
    s = al & ((rank < mn[None, :, None]) | ((rank < mx[None, :, None]) & ~(score < 0)))
    decided = ~(al & (np.abs(score) < MARGIN)).any((1, 2))
    srt = np.take_along_axis(np.where(al, score, -np.inf), order, axis=-1)      # [G,4,32] the allowed scores, descending
    n_al = allowed.sum(-1)
    for k in range(4):
        if 0 < mn[k] < n_al[k]:
            decided &= ~((srt[:, k, mn[k]] < 0) & (srt[:, k, mn[k] - 1] - srt[:, k, mn[k]] < MARGIN))
        if 0 < mx[k] < n_al[k]:
            decided &= ~(~(srt[:, k, mx[k] - 1] < 0) & (srt[:, k, mx[k] - 1] - srt[:, k, mx[k]] < MARGIN))
    empty = ~s.any((1, 2))
    cand = np.where(al & (mx > 0)[None, :, None], score, -np.inf).reshape(G, 128)
    best = cand.argmax(1)                                                        # numpy: the first of equal maxima
    top2 = np.sort(cand, axis=1)[:, -2:]
    decided &= ~(empty & (top2[:, 1] - top2[:, 0] < MARGIN))
    s = s.reshape(G, 128)
    s[empty, best[empty]] = True
    s = s.reshape(G, 4, 32)
    return s, s.sum(-1), decided, empty


def device(x, T, seed, r, **kw):
    return ops.sample_structure(x.to(DEV), T, seed=seed, return_counts=True, **r, **kw)


def check_invariants(s_u8, counts, r, what=None):
    """On every bar, decided or not: 0/1, nothing outside the mask, the counts inside the bounds (max_active + 1 only on a track
    with min_active 0 of a bar that holds that one cell alone), no empty bar, track_count = the sums."""
    _, mn, mx, allowed = rules_of(r)
    assert np.isin(s_u8, (0, 1)).all(), what
    s = s_u8.astype(bool)
    assert not (s & ~allowed[None]).any(), what
    n = s.sum(-1)
    total = n.sum(-1, keepdims=True)
    assert np.array_equal(counts, n), what
    assert (total >= 1).all(), what
    assert ((n >= mn) & ((n <= mx) | ((n == mx + 1) & (mn == 0) & (total == 1)))).all(), what


def c_rules(T, r):
    """the host struct of a rule set, for calls of the C entry itself"""
    bias, mn, mx, allowed = rules_of(r)
    rules = _lib.PmStructureRules()
    rules.temperature = T
    for k in range(4):
        rules.bias[k], rules.min_active[k], rules.max_active[k] = bias[k], int(mn[k]), int(mx[k])
        rules.step_mask[k] = int((allowed[k].astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum())
    return rules


_CASES = {}


def case(G, li, ti, ri):
    """(logits, device s as uint8, device counts, replica s, replica counts, decided, empty) of one case, computed once"""
    key = (G, li, ti, ri)
    if key not in _CASES:
        x, r, seed = make_logits(G, li), RULE_SETS[ri], 4000 + 100 * li + 10 * ti + ri
        s, cnt = device(x, TEMPS[ti], seed, r)
        assert s.shape == (G, 4, 32) and s.dtype == torch.bool and cnt.shape == (G, 4) and cnt.dtype == torch.int32
        _CASES[key] = (x, s.view(torch.uint8).cpu().numpy(), cnt.cpu().numpy()) + replica(x.numpy(), TEMPS[ti], seed, *rules_of(r))
    return _CASES[key]


ALL_CASES = [(li, ti, ri) for li in range(len(LOGITS)) for ti in range(len(TEMPS)) for ri in range(len(RULE_SETS))]


@pytest.mark.parametrize("G", SIZES)
def test_structure_equals_the_fp64_replica(G):
    """Every decided bar bit for bit, in s_u8, s_f32 and track_count.  At G = 515 at most 5 % of the bars may be left out: the
    replica alone (nothing of the device enters that) leaves out at most 0.0098 of them at exactly these inputs."""
    fallbacks = outside0 = 0
    for li, ti, ri in ALL_CASES:
        x, got, got_n, want, want_n, decided, empty = case(G, li, ti, ri)
        left_out = 1.0 - decided.mean()
        differ = int(((got.astype(bool) != want).any((1, 2)) | (got_n != want_n).any(1))[decided].sum())
        print(f"G={G} logits={LOGITS[li]} T={TEMPS[ti]} rules={ri}: {left_out:.4f} of the bars left out, {int(empty.sum())} fallbacks, "
              f"{differ} decided bars differ")
        if G == 515:
            assert left_out <= LEFT_OUT_CAP, (li, ti, ri, left_out)
        assert np.array_equal(got.astype(bool)[decided], want[decided]), (G, li, ti, ri, np.flatnonzero((got.astype(bool) != want).any((1, 2)) & decided)[:8])
        assert np.array_equal(got_n[decided], want_n[decided]), (G, li, ti, ri)
        check_invariants(got, got_n, RULE_SETS[ri], (G, li, ti, ri))
        fallbacks += int((empty & decided).sum())
        outside0 += int((empty & decided & ~want[:, 0].any(-1)).sum())
        if ri == 1 and ti == 0:                        # both outputs of one call: the float form holds the same 0 / 1
            rules, xd = c_rules(TEMPS[ti], RULE_SETS[ri]), x.to(DEV)
            f32, u8 = torch.empty(G, 4, 32, device=DEV), torch.empty(G, 4, 32, dtype=torch.uint8, device=DEV)
            _lib.call("pm_sample_structure", xd.data_ptr(), G, ctypes.addressof(rules), 4000 + 100 * li + 10 * ti + ri, f32.data_ptr(),
                      u8.data_ptr(), None, _lib.stream())
            assert np.array_equal(u8.cpu().numpy(), got) and np.array_equal(f32.cpu().numpy(), got.astype(np.float32))
    if G == 515:
        print(f"{fallbacks} decided empty-bar fallbacks, {outside0} of them outside track 0")
        assert fallbacks > 500 and outside0 > 100      # the no-empty-bar step is exercised, also away from the drums


def test_forced_cells_and_the_fallback_outside_the_drums_occur():
    """What the cases are there for: min_active forcing cells of negative score on, ties aside, and a fallback in tracks 1 and 3."""
    forced = 0
    for li, ti in ((2, 0), (2, 2)):
        x, got, got_n, want, want_n, decided, empty = case(515, li, ti, 1)
        forced += int((got_n[:, 0] == 2).sum())
        assert (got_n[:, 3] == 4).all() and (got[:, 3, ::8] == 1).all()          # min = max = the four allowed steps
        x, got, got_n, want, want_n, decided, empty = case(515, li, ti, 2)
        assert (got_n[:, 0] == 0).all() and (got_n[:, 2] == 0).all()             # muted
        assert (got_n[empty & decided].sum(-1) == 1).all()
        assert (got_n[empty & decided][:, 1] == 1).any() and (got_n[empty & decided][:, 3] == 1).any()
    assert forced > 500


def test_structure_is_a_pure_function_of_seed_bar_and_cell():
    for li, ti, ri in ((0, 2, 0), (1, 1, 1), (2, 3, 2), (1, 0, 1)):
        big, small, one = case(515, li, ti, ri), case(3, li, ti, ri), case(1, li, ti, ri)
        assert np.array_equal(big[1][:3], small[1]) and np.array_equal(big[2][:3], small[2])
        assert np.array_equal(big[1][:1], one[1]) and np.array_equal(big[2][:1], one[2])
        x, r, seed = big[0], RULE_SETS[ri], 4000 + 100 * li + 10 * ti + ri
        s, cnt = device(x, TEMPS[ti], seed, r)
        assert np.array_equal(s.view(torch.uint8).cpu().numpy(), big[1]) and np.array_equal(cnt.cpu().numpy(), big[2])
        # the bars are numbered along the flattened leading dimensions
        s5, cnt5 = device(x[:510].reshape(5, 102, 4, 32), TEMPS[ti], seed, r)
        assert s5.shape == (5, 102, 4, 32) and cnt5.shape == (5, 102, 4)
        assert np.array_equal(s5.view(torch.uint8).cpu().numpy().reshape(510, 4, 32), big[1][:510])
    x, got = case(515, 0, 2, 0)[:2]
    other, _ = device(x, 1.0, 4021, RULE_SETS[0])
    assert not np.array_equal(other.view(torch.uint8).cpu().numpy(), got)
    plain = ops.sample_structure(x.to(DEV), 1.0, seed=4020)
    assert plain.dtype == torch.bool and np.array_equal(plain.view(torch.uint8).cpu().numpy(), got)


@pytest.mark.parametrize("G", SIZES)
def test_no_noise_and_default_rules_give_the_thresholded_structure(G):
    for li in range(len(LOGITS)):
        x = make_logits(G, li)
        assert float(x.abs().min()) >= 1e-6
        want = ops.binary_from_logits(x.to(DEV), 0.5).cpu().numpy()
        got = ops.sample_structure(x.to(DEV), 0.0, seed=li).cpu().numpy()
        nonempty = (x.numpy() >= 0).any((1, 2))
        assert np.array_equal(got[nonempty], want[nonempty]) and np.array_equal(want[nonempty], x.numpy()[nonempty] >= 0)
        assert (got[~nonempty].sum((1, 2)) == 1).all()
        if G == 515 and li == 2:                       # P(a cell >= 0) = 0.0038: about 0.61 of the bars are empty
            assert nonempty.sum() > 100 and (~nonempty).sum() > 200
        # the seed has no say without noise
        assert np.array_equal(ops.sample_structure(x.to(DEV), 0.0, seed=77).cpu().numpy(), got)


@pytest.mark.parametrize("i,x,T,th", [(0, 0.7, 1.3, .5), (1, -1.5, 0.6, .5), (2, 0.2, 1.0, .3), (3, 2.0, 2.0, .7)])
def test_share_of_active_cells_follows_the_sigmoid(i, x, T, th):
    n = 515 * 128
    logits = torch.full((515, 4, 32), x, device=DEV)
    s = ops.sample_structure(logits, T, threshold=th, seed=31 + i)
    share = float(s.float().mean())
    bias = float(np.float32(math.log(th / (1.0 - th))))
    p = 1.0 / (1.0 + math.exp(-(x - bias) / T))
    sigma = (p * (1.0 - p) / n) ** 0.5
    print(f"x={x} T={T} threshold={th}: share {share:.5f}, expected {p:.5f}, {(share - p) / sigma:+.2f} sigma")
    assert abs(share - p) <= 5.0 * sigma, (share, p, sigma)


def test_non_finite_logits_keep_the_invariants_and_touch_nothing_else():
    G, pad, canary = 3, 9, 0x5A
    nan, inf = float("nan"), float("inf")
    x = torch.randn(G, 4, 32, generator=torch.Generator().manual_seed(8))
    x[0, 0, 3], x[0, 0, 4], x[0, 0, 9] = nan, inf, -inf
    x[0, 1] = nan
    x[0, 2, ::2], x[0, 2, 1::2] = inf, -inf
    x[0, 3, 8], x[0, 3, 16] = -inf, nan
    x[1] = -inf
    x[2] = nan
    x[2, 0, :4] = torch.tensor([inf, -inf, 3.0e38, -3.0e38])
    r = RULE_SETS[1]
    for T in (0.0, 1.0, 1e-30, 1e30):
        rules, xd = c_rules(T, r), x.to(DEV)
        b8 = torch.full((pad + G * 128 + pad,), canary, dtype=torch.uint8, device=DEV)
        bf = torch.full((pad + G * 128 + pad,), -7.0, device=DEV)
        bc = torch.full((pad + G * 4 + pad,), -7, dtype=torch.int32, device=DEV)
        _lib.call("pm_sample_structure", xd.data_ptr(), G, ctypes.addressof(rules), 5, bf.data_ptr() + 4 * pad, b8.data_ptr() + pad,
                  bc.data_ptr() + 4 * pad, _lib.stream())
        o8, of, oc = b8.cpu().numpy(), bf.cpu().numpy(), bc.cpu().numpy()
        for o, c in ((o8, canary), (of, -7.0), (oc, -7)):
            assert (o[:pad] == c).all() and (o[-pad:] == c).all(), T
        s8, cnt = o8[pad:-pad].reshape(G, 4, 32), oc[pad:-pad].reshape(G, 4)
        assert np.array_equal(of[pad:-pad].reshape(G, 4, 32), s8.astype(np.float32)), T
        check_invariants(s8, cnt, r, T)
        s, cnt2 = ops.sample_structure(xd, T, seed=5, return_counts=True, **r)
        assert np.array_equal(s.view(torch.uint8).cpu().numpy(), s8) and np.array_equal(cnt2.cpu().numpy(), cnt)
        for rr in (RULE_SETS[0], RULE_SETS[2]):
            s, cnt2 = ops.sample_structure(xd, T, seed=5, return_counts=True, **rr)
            check_invariants(s.view(torch.uint8).cpu().numpy(), cnt2.cpu().numpy(), rr, T)
    s, cnt = ops.sample_structure(x[:0].to(DEV), return_counts=True)
    assert s.shape == (0, 4, 32) and s.dtype == torch.bool and cnt.shape == (0, 4) and cnt.dtype == torch.int32
    with pytest.raises(_lib.HipExtensionError):
        ops.sample_structure(x)                         # a host tensor: no CPU fallback
    with pytest.raises(TypeError):
        ops.sample_structure(x.double().to(DEV))
    with pytest.raises(ValueError):
        ops.sample_structure(x.reshape(G, 32, 4).to(DEV))


# ---- end to end -----------------------------------------------------------------------------------------------------------
E2E = dict(temperature=1.0, threshold=(.5, .4, .6, .5), min_active=(1, 0, 0, 2), max_active=(12, 16, 8, 4),
           allowed_steps=np.stack([step_mask(), step_mask(2), step_mask(), step_mask(4)]))
E2E_RULES = StructureRules(**E2E)
SEED = 7
CHORDS = dict(min_notes=(1, 1, 2, 0), max_notes=(14, 1, 6, 14),
              allowed_pitches=np.stack([pitch_mask(), pitch_mask(28, 60), pitch_mask(40, 88, (0, 2, 4, 5, 7, 9, 11)), pitch_mask(60, 62)]))


@pytest.mark.parametrize("name", ["lmd2_tiny", "nb3_tiny"])
def test_generate_music_with_structure_rules_end_to_end(name):
    z, cfg = load_case(name)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    nb = cfg["n_bars"]
    zs = torch.randn(1, cfg["d"], generator=torch.Generator().manual_seed(11)).repeat(4, 1).to(DEV)     # four takes on one latent
    r = {k: v for k, v in E2E.items() if k != "temperature"}
    with torch.no_grad():
        s_logits = vae.engine.structure_only(zs, False).detach().contiguous().float()
        assert s_logits.shape == (4, nb, 4, 32)
        want_s, want_n = ops.sample_structure(s_logits, 1.0, seed=SEED, return_counts=True, **r)
        mtp, s_tensor = generate_music(vae, zs, structure_rules=E2E_RULES, seed=SEED)
        assert s_tensor.dtype == torch.bool and torch.equal(s_tensor, want_s) and mtp.shape == (4, nb, 4, 32, 15, 230)
        # the replica on the model's logits: the rows of the repeated latent differ, and the device drew the decided bars
        rep_s, rep_n, decided, _ = replica(s_logits.reshape(-1, 4, 32).cpu().numpy(), 1.0, SEED, *rules_of(r))
        rep_rows = rep_s.reshape(4, -1)
        assert all(not np.array_equal(rep_rows[0], rep_rows[b]) for b in range(1, 4))
        got = s_tensor.reshape(-1, 4, 32).cpu().numpy()
        assert np.array_equal(got[decided], rep_s[decided]) and decided.mean() >= 0.5
        assert all(not torch.equal(s_tensor[0], s_tensor[b]) for b in range(1, 4))
        check_invariants(got.astype(np.uint8), want_n.reshape(-1, 4).cpu().numpy(), r)
        # the active cells of the pianoroll are exactly the drawn structure: a silent cell is one-hot EOS / PAD with no duration
        silent = (mtp[..., 131:].abs().sum((-1, -2)) == 0) & (mtp[..., 0, 129] == 1) & (mtp[..., 1:, 130] == 1).all(-1) & \
                 (mtp.abs().sum((-1, -2)) == 15)
        assert torch.equal(~silent, s_tensor)
        # the content decoder ran on the drawn structure
        graph = vae.decoder._structure_from_binary(s_tensor.clone())
        _, c_logits = vae.decoder(zs, graph)
        c_logits = c_logits.detach().contiguous().float()
        assert c_logits.shape[0] == int(s_tensor.sum())
        assert torch.equal(mtp, ops.mtp_from_logits(c_logits, s_tensor))
        # the same call again is the same pianoroll, bit for bit; seed=None repeats under torch.manual_seed
        again = generate_music(vae, zs, structure_rules=E2E_RULES, seed=SEED)
        assert torch.equal(again[0], mtp) and torch.equal(again[1], s_tensor)
        torch.manual_seed(99)
        a = generate_music(vae, zs, structure_rules=E2E_RULES, temperature=1.0)
        torch.manual_seed(99)
        b = generate_music(vae, zs, structure_rules=E2E_RULES, temperature=1.0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[1], s_tensor)
        # sampled tokens on the sampled structure: one seed, the streams kept apart by the head
        mtp_t, s_t, tokens = generate_music(vae, zs, structure_rules=E2E_RULES, seed=SEED, temperature=0.9, top_k=20, return_tokens=True)
        assert torch.equal(s_t, s_tensor) and torch.equal(tokens, ops.sample_tokens(c_logits, 0.9, 20, None, SEED))
        assert torch.equal(mtp_t, ops.mtp_from_tokens(tokens, s_tensor))
        # chords on the sampled structure
        mtp_c, s_c, tok_c, notes = generate_music(vae, zs, structure_rules=E2E_RULES, seed=SEED, chord_rules=ChordRules(**CHORDS),
                                                  return_tokens=True, return_note_counts=True)
        N = int(s_tensor.sum())
        assert torch.equal(s_c, s_tensor) and tok_c.shape == (N, 15, 2) and notes.shape == (N,)
        track = ops.node_tracks(s_tensor, N)
        assert torch.equal(track.cpu(), s_tensor.reshape(-1, 4, 32).nonzero()[:, 1].to(torch.uint8).cpu())
        want_tok, want_notes = ops.sample_chords(c_logits, track, seed=SEED, **CHORDS)
        assert torch.equal(tok_c, want_tok) and torch.equal(notes, want_notes)
        tr, nn = track.cpu().numpy(), notes.cpu().numpy()
        assert (nn >= np.array(CHORDS["min_notes"])[tr]).all() and (nn <= np.array(CHORDS["max_notes"])[tr]).all()
        assert torch.equal(mtp_c, ops.mtp_from_tokens(tok_c, s_tensor))
        # without the keyword the call is what it was: the thresholded structure and the logits on it
        mtp0, s0 = generate_music(vae, zs)
        mtp1, s1 = generate_music(vae, zs, structure_rules=None)
        assert torch.equal(s0, s1) and torch.equal(mtp0, mtp1)
        assert torch.equal(s0, ops.binary_from_logits(s_logits, 0.5))
        _, c0 = vae.decoder(zs, vae.decoder._structure_from_binary(s0.clone()))
        assert torch.equal(mtp0, ops.mtp_from_logits(c0.detach().contiguous().float(), s0))
        assert all(torch.equal(s0[0], s0[b]) for b in range(1, 4))               # one latent, one rhythm: the gap this closes
        # no noise and default rules: the thresholded structure wherever its bar is not empty
        s_t0 = generate_music(vae, zs, structure_rules=StructureRules(temperature=0), seed=SEED)[1]
        nonempty = (s_logits.reshape(-1, 128) >= 0).any(-1)                      # (s0 itself holds the [0,0] of an empty bar)
        assert float(s_logits.abs().min()) >= 1e-6
        assert torch.equal(s_t0.reshape(-1, 128)[nonempty], s0.reshape(-1, 128)[nonempty])
