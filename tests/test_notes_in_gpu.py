"""Notes in on the device (csrc/notes_in.hip, `ops.tokens_from_notes`, `graphs.device_batch_from_notes`, `NoteBatch.from_lists` /
`to_graph`, `generate.encode_notes` / `vary_notes`) against the numpy restatement of the reference's preprocessing
(`tokens_ref`, tests/notes_in_util.py, which tests/test_notes_in_abi.py ties to the golden cases) and against the other
direction, `ops.notes_from_tokens`.  Integers throughout: every comparison is exact, the structure tensor bit for bit."""
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import ChordRules, NoteBatch, StructureRules, encode_notes, generate_notes, vary_notes
from polyphemus_amd.graphs import device_batch_from_notes, device_batch_from_structure
from polyphemus_amd.model import VAE
from notes_in_util import as_batch, check_ref, end_clamped, tokens_ref
from notes_util import CASES
from test_graphs_gpu import assert_same, host_batch
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -123456789


def chord(t, n, base=30):
    """n notes at time t, pitches in an order that is neither ascending nor descending, durations 1..n"""
    return [(t, base + (7 * j) % 50, 1 + j) for j in range(n)]


def hand_made(B, n_bars, seed=0):
    """pieces as lists.  Piece 0 by hand: cells of 1, 14, 15 and 20 notes (1 + 6 dropped), notes at time 0 and at the last step,
    pitches -3 and 200, durations 0, 1, 96, 97 and 500, an empty track (Bass), equal times in a chosen order; with three bars
    the middle one is empty.  Piece 1 (B > 1) has no note at all, the others are drawn."""
    L = 32 * n_bars
    rng = np.random.default_rng(seed)
    pieces = [[[], [], [], []] for _ in range(B)]
    pieces[0][0] = [(0, 36, 0)] + chord(5, 14) + [(9, 40, 96), (L - 1, -3, 500)]
    pieces[0][2] = chord(7, 15) + [(L - 1, 200, 97), (L - 1, 0, 1), (L - 1, 127, 96)]
    pieces[0][3] = [(0, 72, 1), (0, 60, 1), (0, 67, 1)] + chord(31, 20, base=60)
    for i in range(2, B):
        for k in range(4):
            n = int(rng.integers(0, 40))
            times = np.sort(rng.integers(0, L, n))
            pieces[i][k] = [(int(t), int(rng.integers(-5, 135)), int(rng.integers(-2, 110))) for t in times]
    return pieces


def device_tokens(notes, ptr, n_bars, **kw):
    """(s_tensor, tokens, info) as numpy, after the checks every result must pass"""
    s, tok, info = ops.tokens_from_notes(torch.from_numpy(notes).to(DEV), torch.from_numpy(ptr).to(DEV), n_bars, **kw)
    G = (len(ptr) - 1) // 4 * n_bars
    assert s.dtype == torch.float32 and s.shape == (G, 4, 32) and s.is_cuda and s.is_contiguous()
    assert tok.dtype == torch.int32 and tok.shape == (info["num_nodes"], 16, 2) and tok.is_cuda and tok.is_contiguous()
    assert set(info) == {"dropped", "out_of_range", "out_of_order", "bad_track_ptr", "num_nodes"}
    assert int(s.sum()) == info["num_nodes"]
    return s.cpu().numpy(), tok.cpu().numpy(), info


def assert_equals_ref(notes, ptr, n_bars):
    s, tok, info = device_tokens(notes, ptr, n_bars)
    want_s, want_tok, dropped = tokens_ref(notes, ptr, n_bars)
    assert s.tobytes() == want_s.tobytes()
    assert tok.shape == want_tok.shape and np.array_equal(tok, want_tok), np.flatnonzero((tok != want_tok).any((1, 2)))[:8]
    assert info["dropped"] == dropped and info["out_of_range"] == info["out_of_order"] == info["bad_track_ptr"] == 0
    return s, tok, info


@pytest.mark.parametrize("B,n_bars", [(1, 1), (3, 2), (5, 3)])
def test_hand_made_batches_equal_the_restatement(B, n_bars):
    """G = 1, 6 and 15 bars (odd: the bar-count kernel's last half-wave has no bar, the last block of the bar-per-wave kernels
    holds waves without one)"""
    pieces = hand_made(B, n_bars)
    notes, ptr = as_batch(pieces)
    s, tok, info = assert_equals_ref(notes, ptr, n_bars)
    L = 32 * n_bars
    s5 = s.reshape(B, n_bars, 4, 32)
    node = (np.cumsum(s5.reshape(-1)) - 1).astype(np.int64).reshape(s5.shape)
    cell = lambda i, k, t: tok[node[i, t // 32, k, t % 32]]
    PAD, EOS = [130, 98], [129, 97]
    # one note, duration 0 -> token 0; time 0
    assert cell(0, 0, 0).tolist() == [[128, 96], [36, 0], EOS] + [PAD] * 13
    # 14 notes fill the slots 1..14 in list order, EOS in slot 15; 15 and 20 notes: the same, the later ones dropped
    assert cell(0, 0, 5).tolist() == [[128, 96]] + [[p, d - 1] for (_, p, d) in chord(5, 14)] + [EOS]
    assert cell(0, 2, 7).tolist() == [[128, 96]] + [[p, d - 1] for (_, p, d) in chord(7, 15)[:14]] + [EOS]
    assert cell(0, 3, 31).tolist() == [[128, 96]] + [[p, d - 1] for (_, p, d) in chord(31, 20, 60)[:14]] + [EOS]
    assert cell(0, 0, L - 1).tolist() == [[128, 96], [0, 95], EOS] + [PAD] * 13           # pitch -3, duration 500
    # the last step: pitches 200, 0, 127 and durations 97, 1, 96, in list order; equal times keep the list order
    assert cell(0, 2, L - 1).tolist() == [[128, 96], [127, 95], [0, 0], [127, 95], EOS] + [PAD] * 11
    assert cell(0, 3, 0).tolist()[:5] == [[128, 96], [72, 0], [60, 0], [67, 0], EOS]
    assert cell(0, 0, 9).tolist()[:3] == [[128, 96], [40, 95], EOS]
    assert not s5[0, :, 1].any()                                                          # the empty track
    if B == 1:
        assert info["dropped"] == 7
    else:
        assert info["dropped"] >= 7 and not s5[1, :, :, :].reshape(n_bars, -1)[:, 1:].any()   # the piece without notes ...
        assert (s5[1, :, 0, 0] == 1).all() and (tok[node[1, :, 0, 0]] == [[128, 96], EOS] + [PAD] * 14).all()   # ... one silent cell a bar
    if n_bars == 3:                                                                       # the empty bar between full ones
        assert s5[0, 1].sum() == 1 and cell(0, 0, 32).tolist() == [[128, 96], EOS] + [PAD] * 14


@pytest.mark.parametrize("B,n_bars", [(1, 1), (3, 2)])
def test_no_notes_at_all(B, n_bars):
    notes, ptr = np.zeros((0, 3), np.int32), np.zeros(4 * B + 1, np.int32)
    s, tok, info = assert_equals_ref(notes, ptr, n_bars)
    assert info["num_nodes"] == B * n_bars and info["dropped"] == 0 and s.sum() == B * n_bars and (s[:, 0, 0] == 1).all()
    nb = NoteBatch.from_lists([[[], [], [], []]] * B, n_bars, device=DEV)
    assert nb.notes.shape == (0, 3) and nb.to_graph().num_nodes == B * n_bars


# ---- there and back ---------------------------------------------------------------------------------------------------------
def chord_form(B, n_bars, p, seed):
    """seeded (tokens int32 [N,15,2], s bool [B,n_bars,4,32]): no empty bar; every node 1..14 notes, then EOS, then PAD"""
    rng = np.random.default_rng(seed)
    s = rng.random((B, n_bars, 4, 32)) < p
    for i, b in np.argwhere(~s.any(axis=(2, 3))):
        s[i, b, rng.integers(0, 4), rng.integers(0, 32)] = True
    N = int(s.sum())
    count = rng.integers(1, 15, N)
    tokens = np.stack([rng.integers(0, 128, (N, 15)), rng.integers(0, 96, (N, 15))], -1).astype(np.int32)
    slot = np.arange(15)[None, :]
    tokens[slot == count[:, None]] = (129, 97)
    tokens[slot > count[:, None]] = (130, 98)
    return tokens, s


def assert_round_trip(tokens15, s, n_bars):
    """tokens [N,15,2] (device) on the structure s [B,n_bars,4,32] (device) -> notes -> structure and tokens again"""
    notes, track_ptr, totals = ops.notes_from_tokens(tokens15, s)
    s2, tok2, info = ops.tokens_from_notes(notes, track_ptr, n_bars)
    sos = torch.tensor([128, 96], dtype=torch.int32, device=DEV).expand(tokens15.shape[0], 1, 2)
    want = end_clamped(torch.cat([sos, tokens15], 1).cpu().numpy(), s.cpu().numpy(), n_bars)
    assert s2.cpu().numpy().tobytes() == s.reshape(-1, 4, 32).float().cpu().numpy().tobytes()
    assert np.array_equal(tok2.cpu().numpy(), want)
    assert info == dict(dropped=0, out_of_range=0, out_of_order=0, bad_track_ptr=0, num_nodes=tokens15.shape[0])
    return notes, track_ptr, totals


@pytest.mark.parametrize("B,n_bars,p", [(4, 2, 0.3), (7, 3, 0.15), (2, 1, 1.0), (260, 4, 0.04)],
                         ids=["even-bars", "odd-bars", "every-cell", "1040-bars"])
def test_round_trip_of_drawn_chords(B, n_bars, p):
    """1040 bars: more than the scan's 1024 threads"""
    tokens, s = chord_form(B, n_bars, p, 17 * B + n_bars)
    assert_round_trip(torch.from_numpy(tokens).to(DEV), torch.from_numpy(s).to(DEV), n_bars)


@pytest.mark.parametrize("name", list(CASES))
def test_round_trip_of_the_golden_batches(name):
    B, n_bars = CASES[name]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    tokens = torch.from_numpy(z["in/tokens"].astype(np.int32)[:, 1:].copy()).to(DEV)
    s = torch.from_numpy(z["in/s_tensor"].reshape(B, n_bars, 4, 32)).to(DEV)
    assert_round_trip(tokens, s, n_bars)


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
    """a generated NoteBatch (chord rules: every active cell holds a note), its structure and tokens"""
    vae, zs, _ = model
    with torch.no_grad():
        return generate_notes(vae, zs, chord_rules=ChordRules(), seed=3, return_tokens=True)


def test_round_trip_of_a_generated_batch(model, take):
    batch, s_tensor, tokens = take
    notes, track_ptr, _ = assert_round_trip(tokens, s_tensor, model[2])
    assert torch.equal(track_ptr, batch.track_ptr) and torch.equal(notes[:int(track_ptr[-1])], batch.notes[:int(track_ptr[-1])])
    # ... and through the lists
    again = NoteBatch.from_lists(batch.tolist(), batch.n_bars, device=DEV)
    M = int(batch.totals[0])
    assert torch.equal(again.notes, batch.notes[:M]) and torch.equal(again.track_ptr, batch.track_ptr)
    assert torch.equal(again.totals, batch.totals)
    g1, g2 = batch.to_graph(), again.to_graph()
    assert torch.equal(g1.tokens, g2.tokens) and torch.equal(g1.s_tensor, g2.s_tensor) and torch.equal(g1.edge_index, g2.edge_index)
    assert torch.equal(g1.s_tensor.view(s_tensor.shape).bool(), s_tensor)


# ---- safety -----------------------------------------------------------------------------------------------------------------
def raw(notes, ptr, n_bars, cap, pad=64):
    """pm_tokens_from_notes through the raw binding, every output in front of `pad` sentinel words: (s_tensor, tokens, scratch,
    status) as numpy, pads included, after the check that every pad is intact"""
    B = (len(ptr) - 1) // 4
    G, M = B * n_bars, len(notes)
    n_scratch = 3 * G + 1 + 12 * B
    nd, pd = torch.from_numpy(notes).to(DEV), torch.from_numpy(ptr).to(DEV)
    s = torch.full((128 * G + pad,), float(SENTINEL), dtype=torch.float32, device=DEV)
    tok = torch.full((32 * cap + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    scratch = torch.full((n_scratch + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    status = torch.full((5 + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.call("pm_tokens_from_notes", nd.data_ptr() if M else None, pd.data_ptr(), B, n_bars, M, s.data_ptr(),
              tok.data_ptr() if cap else None, cap, scratch.data_ptr(), status.data_ptr(), _lib.stream())
    out = [t.cpu().numpy() for t in (s, tok, scratch, status)]
    for a, n in zip(out, (128 * G, 32 * cap, n_scratch, 5)):
        assert (a[n:] == a.dtype.type(SENTINEL)).all() and len(a) == n + pad
    return out


def test_canaries_capacity_and_two_calls_write_the_same_bytes():
    n_bars = 3
    notes, ptr = as_batch(hand_made(5, n_bars))
    want_s, want_tok, dropped = tokens_ref(notes, ptr, n_bars)
    N, G = len(want_tok), 15
    for cap in (N, N + 9, len(notes) + G):
        s, tok, scratch, status = raw(notes, ptr, n_bars, cap)
        assert status[:5].tolist() == [0, 0, 0, dropped, N]
        assert s[:128 * G].tobytes() == want_s.tobytes() and np.array_equal(tok[:32 * N].reshape(N, 16, 2), want_tok)
        assert (tok[32 * N:] == SENTINEL).all()                       # rows behind the last node are not written
        again = raw(notes, ptr, n_bars, cap)
        assert all(a.tobytes() == b.tobytes() for a, b in zip((s, tok, scratch, status), again))
    # fewer rows than nodes: the nodes at `capacity` and beyond are not written, the count still says how many there are
    for cap in (N - 5, 1, 0):
        s, tok, scratch, status = raw(notes, ptr, n_bars, cap)
        assert status[:5].tolist() == [0, 0, 0, dropped, N] and s[:128 * G].tobytes() == want_s.tobytes()
        assert np.array_equal(tok[:32 * cap].reshape(cap, 16, 2), want_tok[:cap])


def bad_inputs():
    """(name, notes, track_ptr, the kind that must be named): ordinary bad arguments"""
    n_bars = 2
    notes, ptr = as_batch(hand_made(3, n_bars, seed=5))
    M, L = len(notes), 32 * n_bars
    out = []
    a = notes.copy()                                                  # two rows of the last track swapped: one descent, or two
    lo, hi = int(ptr[-2]), int(ptr[-1])
    assert hi - lo > 8 and a[lo + 2, 0] != a[lo + 6, 0]
    a[[lo + 2, lo + 6]] = a[[lo + 6, lo + 2]]
    out.append(("swapped-rows", a, ptr, "out of order"))
    a = notes.copy()
    a[lo:hi] = a[lo:hi][::-1]                                          # a whole track backwards
    out.append(("reversed-track", a, ptr, "out of order"))
    a = notes.copy()
    a[int(ptr[8]), 0] = -1                                            # the first row of a track: still in order
    a[hi - 1, 0] = L                                                  # the last row of a track: still in order
    out.append(("times-outside", a, ptr, "out of range"))
    a = notes.copy()
    a[hi - 1, 0] = 2 ** 31 - 1
    a[int(ptr[8]), 0] = -2 ** 31
    out.append(("times-at-the-int32-ends", a, ptr, "out of range"))
    p = ptr.copy()
    assert p[1] > 1
    p[2] = p[1] - 1
    out.append(("track_ptr-decreases", notes, p, "track_ptr"))
    p = ptr.copy()
    p[-1] = M + 5
    out.append(("track_ptr-overshoots", notes, p, "track_ptr"))
    p = ptr.copy()
    p[0], p[3], p[4], p[7] = 1, 2 ** 31 - 1, -2 ** 31, -1
    out.append(("track_ptr-anything", notes, p, "track_ptr"))
    return n_bars, out


@pytest.mark.parametrize("case", bad_inputs()[1], ids=lambda c: c[0])
def test_bad_input_is_counted_never_followed(case):
    n_bars = bad_inputs()[0]
    _, notes, ptr, kind = case
    want = dict(zip(("out_of_range", "out_of_order", "bad_track_ptr"), check_ref(notes, ptr, n_bars)))
    count = want[{"out of range": "out_of_range", "out of order": "out_of_order", "track_ptr": "bad_track_ptr"}[kind]]
    assert count > 0
    nd, pd = torch.from_numpy(notes).to(DEV), torch.from_numpy(ptr).to(DEV)
    with pytest.raises(ValueError, match=f"{count} (rows|bad entries)") as e:
        ops.tokens_from_notes(nd, pd, n_bars)
    assert kind in str(e.value)
    with pytest.raises(ValueError, match=kind):
        device_batch_from_notes(nd, pd, n_bars)
    G, cap = 3 * n_bars, len(notes) + 3 * n_bars
    s, tok, scratch, status = raw(notes, ptr, n_bars, cap)            # (its pads are checked)
    assert status[:3].tolist() == [want["out_of_range"], want["out_of_order"], want["bad_track_ptr"]]
    assert np.isin(s[:128 * G], (0.0, 1.0)).all() and 0 <= status[4] <= 128 * G
    again = raw(notes, ptr, n_bars, cap)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((s, tok, scratch, status), again))
    if kind != "track_ptr":                                           # without the check: counted in info, nothing raised
        info = ops.tokens_from_notes(nd, pd, n_bars, check=False)[2]
        assert {k: info[k] for k in want} == want


# ---- the batch, the encoder, variations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_bars", [(3, 2), (5, 3)])
def test_device_batch_from_notes_equals_the_batch_built_from_the_token_grid(B, n_bars):
    notes, ptr = as_batch(hand_made(B, n_bars, seed=9))
    want_s, want_tok, _ = tokens_ref(notes, ptr, n_bars)
    got = device_batch_from_notes(torch.from_numpy(notes).to(DEV), torch.from_numpy(ptr).to(DEV), n_bars)
    grid = np.zeros((B * n_bars, 4, 32, 16, 2), np.int32)
    grid[want_s != 0] = want_tok
    want = device_batch_from_structure(torch.from_numpy(want_s).to(DEV), n_bars, token_grid=torch.from_numpy(grid).to(DEV))
    assert set(got.__dict__) == set(want.__dict__) and got.n_slots == 15 and got.track_unique is True
    for k, v in want.__dict__.items():
        if torch.is_tensor(v):
            assert got.__dict__[k].dtype == v.dtype and torch.equal(got.__dict__[k], v), k
        else:
            assert got.__dict__[k] == v, k
    host = host_batch(want_s.copy(), n_bars)
    assert_same(got, host)
    assert got.tokens.shape == (host.num_nodes, 16, 2)


def test_encode_notes_is_the_encoder_in_eval_mode(model, take):
    vae, _, n_bars = model
    batch = take[0]
    try:
        with _lib.deterministic(True):
            vae.train()
            mu, log_var = encode_notes(vae, batch)
            assert vae.training
            vae.eval()
            mu2, log_var2 = encode_notes(vae, batch)
            assert not vae.training
            with torch.no_grad():
                want = vae.encoder(batch.to_graph())
    finally:
        vae.eval()
    assert mu.shape == log_var.shape == (len(batch.track_ptr) // 4, vae.cfg["d"]) and not mu.requires_grad
    for got in ((mu, log_var), (mu2, log_var2)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="n_bars"):
        encode_notes(vae, NoteBatch(batch.notes, batch.track_ptr, batch.totals, n_bars + 1))


def same_take(a, b):
    M = int(a[0].totals[0])
    return (torch.equal(a[0].totals, b[0].totals) and torch.equal(a[0].track_ptr, b[0].track_ptr)
            and torch.equal(a[0].notes[:M], b[0].notes[:M]) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])))


def test_vary_notes(model, take):
    vae, _, n_bars = model
    batch = take[0]
    kw = dict(temperature=0.9, return_tokens=True)
    with _lib.deterministic(True), torch.no_grad():
        mu, log_var = encode_notes(vae, batch)
        # strength 0 is the reconstruction at mu
        rec = vary_notes(vae, batch, strength=0, seed=11, return_z=True, **kw)
        assert torch.equal(rec[3], mu) and same_take(rec[:3], generate_notes(vae, mu, seed=11, **kw))
        # one seed, one take; another seed, another latent
        a = vary_notes(vae, batch, seed=11, return_z=True, **kw)
        b = vary_notes(vae, batch, seed=11, return_z=True, **kw)
        c = vary_notes(vae, batch, seed=12, return_z=True, **kw)
        assert same_take(a, b) and not torch.equal(a[3], c[3]) and not torch.equal(a[3], mu)
        eps = torch.randn(mu.shape, generator=torch.Generator().manual_seed(11)).to(DEV)
        assert torch.equal(a[3], mu + 1.0 * torch.exp(0.5 * log_var) * eps)
        half = vary_notes(vae, batch, strength=0.5, seed=11, return_z=True)
        assert len(half) == 3 and torch.equal(half[2], mu + 0.5 * torch.exp(0.5 * log_var) * eps)
        # the input's own structure: same rhythm, new notes
        graph = batch.to_graph()
        kept = vary_notes(vae, batch, keep_structure=True, seed=11, chord_rules=ChordRules(), **kw)
        assert torch.equal(kept[1].reshape(-1, 4, 32).float(), graph.s_tensor) and kept[1].dtype == torch.bool
        assert kept[2].shape == (graph.num_nodes, 15, 2) and not torch.equal(kept[2], graph.tokens[:, 1:])
        assert torch.equal(kept[0].to_graph().s_tensor, graph.s_tensor)      # chord rules: every cell keeps a note
        assert same_take(kept, vary_notes(vae, batch, keep_structure=True, seed=11, chord_rules=ChordRules(), **kw))
        with pytest.raises(ValueError, match="structure_rules draws the structure itself"):
            vary_notes(vae, batch, keep_structure=True, structure_rules=StructureRules(), seed=11)
        drawn = vary_notes(vae, batch, structure_rules=StructureRules(max_active=(8, 4, 4, 2)), seed=11)
        assert int(drawn[1][:, :, 3].sum(-1).max()) <= 2
