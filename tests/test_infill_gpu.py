"""Infill on the device (csrc/infill.hip, `ops.infill_structure` / `ops.infill_tokens`, `generate.infill_notes`) against the
numpy restatement of its rules (`infill_ref`, tests/infill_util.py, which tests/test_infill_abi.py ties to a golden case).
Integers and 0 / 1 throughout: every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import (ChordRules, StructureRules, encode_notes, generate_notes, infill_notes, region_mask, step_mask,
                                     vary_notes)
from polyphemus_amd.model import VAE
from infill_util import EOS, PAD, infill_ref
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -123456789


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def random_input(B, n_bars, seed, p=0.06):
    """(s_in fp32 [G,4,32] without an empty bar, tokens_in int32 [N_in,16,2], s_model uint8 [G,4,32], some bars of it empty)"""
    rng = np.random.default_rng(seed)
    G = B * n_bars
    s_in = rng.random((G, 4, 32)) < p
    for g in np.flatnonzero(~s_in.any(axis=(1, 2))):
        s_in[g, rng.integers(0, 4), rng.integers(0, 32)] = True
    s_model = (rng.random((G, 4, 32)) < p) * rng.integers(1, 256, (G, 4, 32))
    s_model[rng.integers(0, G)] = 0
    tokens_in = rng.integers(0, 96, (int(s_in.sum()), 16, 2)).astype(np.int32)
    tokens_in[:, 0] = (128, 96)
    return s_in.astype(np.float32), tokens_in, s_model.astype(np.uint8)


def regions(B, n_bars, seed):
    rng = np.random.default_rng(seed)
    shared = rng.random((n_bars, 4, 32)) < 0.5
    return {"none": np.zeros((n_bars, 4, 32), bool), "all": region_mask(n_bars), "track": region_mask(n_bars, tracks=["Guitar"]),
            "bar": region_mask(n_bars, bars=[n_bars - 1]), "steps": region_mask(n_bars, steps=step_mask(lo=5, hi=20)),
            "per-piece": rng.random((B, n_bars, 4, 32)) < 0.5, "shared": shared,
            "shared-expanded": np.broadcast_to(shared, (B, n_bars, 4, 32)).copy()}


def on_device(s_in, tokens_in, s_model, region, seed=0):
    """both wrappers on the device -> (s_out bool, bar_forced, drawn, tokens, status) as numpy; the drawn tokens are seeded"""
    s_in_d, region_d = dev(s_in), dev(region)
    s_out, forced = ops.infill_structure(s_in_d, dev(s_model), region_d)
    G = len(s_in)
    assert s_out.dtype == torch.bool and s_out.shape == (G, 4, 32) and forced.dtype == torch.int32 and forced.shape == (G,)
    N = int(s_out.sum())
    drawn = np.random.default_rng(seed).integers(0, 131, (N, 15, 2)).astype(np.int32)
    tokens = dev(drawn)
    status = ops.infill_tokens(s_in_d, s_out.float(), region_d, dev(tokens_in), tokens, forced)
    assert status.dtype == torch.int32 and status.shape == (5,) and status.is_cuda
    return s_out.cpu().numpy(), forced.cpu().numpy(), drawn, tokens.cpu().numpy(), status.cpu().numpy()


def assert_equals_ref(s_in, tokens_in, s_model, region):
    s_out, forced, drawn, tokens, status = on_device(s_in, tokens_in, s_model, region)
    want_s, want_forced, want_tokens, want_status = infill_ref(s_in, tokens_in, s_model, drawn, region)
    assert np.array_equal(s_out, want_s) and np.array_equal(forced, want_forced)
    assert tokens.shape == want_tokens.shape and np.array_equal(tokens, want_tokens), np.flatnonzero((tokens != want_tokens).any((1, 2)))[:8]
    assert status.tolist() == want_status.tolist() and status[0] == len(drawn)
    return s_out, forced, tokens, status


@pytest.mark.parametrize("kind", ["none", "all", "track", "bar", "steps", "per-piece", "shared"])
@pytest.mark.parametrize("B,n_bars", [(1, 1), (3, 2), (5, 3), (260, 4)])
def test_kernels_equal_the_restatement(B, n_bars, kind):
    """G = 1 (a lone half-wave), 6, 15 (odd: a half-wave and waves of the last block without a bar) and 1040 bars (the scan's
    per-thread run exceeds one, the last blocks are partial)"""
    s_in, tokens_in, s_model = random_input(B, n_bars, 100 * B + n_bars, p=0.03 if B > 100 else 0.06)
    region = regions(B, n_bars, B)[kind]
    s_out, forced, tokens, status = assert_equals_ref(s_in, tokens_in, s_model, region)
    if kind == "none":
        assert np.array_equal(s_out, s_in != 0) and np.array_equal(tokens, tokens_in[:, 1:]) and not forced.any()
    if kind == "all":
        assert status[2] == status[3] == 0 and forced.sum() >= 1          # (s_model has an empty bar)


@pytest.mark.parametrize("B,n_bars", [(3, 2), (5, 3)])
def test_a_shared_region_equals_the_same_mask_expanded(B, n_bars):
    s_in, tokens_in, s_model = random_input(B, n_bars, 7)
    r = regions(B, n_bars, 3)
    a = on_device(s_in, tokens_in, s_model, r["shared"])
    b = on_device(s_in, tokens_in, s_model, r["shared-expanded"])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("inside", [True, False], ids=["cell00-inside", "cell00-outside"])
def test_bars_that_come_out_empty_get_cell_00(inside):
    """s_in active only inside the region, s_model off there: bar 1 of 3 comes out empty and gets [0,0], inside the region
    (its row stays as drawn) or outside (a kept node without a source: the chord of a cell without a note)"""
    G = 3
    s_in = np.zeros((G, 4, 32), np.float32)
    s_in[0, 1, 4] = s_in[1, 0, 9] = s_in[1, 2, 30] = s_in[2, 3, 31] = 1
    if inside:
        s_in[1] = 0
        s_in[1, 0, 0] = s_in[1, 0, 9] = 1
    region = np.zeros((G, 4, 32), bool)
    region[1, 0, 0 if inside else 9] = region[1, 0, 9] = region[1, 2, 30] = True
    s_model = np.zeros((G, 4, 32), np.uint8)
    s_model[0] = 1                                                      # outside the region: ignored
    tokens_in = (20 * np.arange(int(s_in.sum()))[:, None, None] + np.arange(16)[None, :, None] + np.zeros((1, 1, 2))).astype(np.int32)
    s_out, forced, tokens, status = assert_equals_ref(s_in, tokens_in, s_model, region)
    assert forced.tolist() == [0, 1, 0] and s_out.sum() == 3 and s_out[1, 0, 0] and s_out[1].sum() == 1
    drawn = on_device(s_in, tokens_in, s_model, region)[2]
    if inside:
        assert np.array_equal(tokens[1], drawn[1]) and status.tolist() == [3, int(s_in.sum()), 2, 0, 1]
    else:
        assert tokens[1].tolist() == [list(EOS)] + [list(PAD)] * 14 and status.tolist() == [3, 4, 3, 1, 1]
    assert np.array_equal(tokens[0], tokens_in[0, 1:]) and np.array_equal(tokens[2], tokens_in[-1, 1:])


# ---- safety -----------------------------------------------------------------------------------------------------------------
def padded(n, dtype, pad=64):
    return torch.full((n + pad,), SENTINEL if dtype != torch.uint8 else 0xA5, dtype=dtype, device=DEV)


def raw(s_in, tokens_in, s_model, region, drawn, N_in=None, N=None, pad=64):
    """both entries through the raw binding, every output in front of `pad` sentinel words: (s_f32, s_u8, bar_forced, tokens,
    scratch, status) as numpy, pads included, after the check that every pad is intact.  `drawn` fills the tokens buffer,
    N_in / N are what the call is told (default: the buffers' rows)."""
    G, R = len(s_in), region.size // 128
    N_in = len(tokens_in) if N_in is None else N_in
    N = len(drawn) if N is None else N
    s_in_d, s_model_d, region_d, tin = dev(s_in), dev(s_model), dev(region.reshape(-1, 4, 32).astype(np.uint8)), dev(tokens_in)
    s_f32, s_u8, forced = padded(128 * G, torch.float32), padded(128 * G, torch.uint8), padded(G, torch.int32)
    _lib.call("pm_infill_structure", s_in_d.data_ptr(), s_model_d.data_ptr(), region_d.data_ptr(), G, R, s_f32.data_ptr(),
              s_u8.data_ptr(), forced.data_ptr(), _lib.stream())
    tok = padded(30 * len(drawn), torch.int32)
    tok[:30 * len(drawn)] = dev(drawn).reshape(-1)
    scratch, status = padded(6 * G + 2, torch.int32), padded(5, torch.int32)
    s_out = s_f32[:128 * G].clone()
    _lib.call("pm_infill_tokens", s_in_d.data_ptr(), s_out.data_ptr(), region_d.data_ptr(), G, R, tin.data_ptr() if N_in else None,
              N_in, tok.data_ptr() if N else None, N, forced.data_ptr(), scratch.data_ptr(), status.data_ptr(), _lib.stream())
    out = [t.cpu().numpy() for t in (s_f32, s_u8, forced, tok, scratch, status)]
    for a, n in zip(out, (128 * G, 128 * G, G, 30 * len(drawn), 6 * G + 2, 5)):
        assert len(a) == n + pad and (a[n:] == (0xA5 if a.dtype == np.uint8 else a.dtype.type(SENTINEL))).all()
    return out


def test_canaries_short_buffers_and_two_calls_write_the_same_bytes():
    B, n_bars = 5, 3
    G = B * n_bars
    s_in, tokens_in, s_model = random_input(B, n_bars, 21)
    region = regions(B, n_bars, 2)["per-piece"]
    want_s, want_forced, _, _ = infill_ref(s_in, tokens_in, s_model, np.zeros((0, 15, 2)), region)
    cells, N_in = int(want_s.sum()), len(tokens_in)
    drawn = np.random.default_rng(1).integers(0, 131, (cells + 9, 15, 2)).astype(np.int32)
    # every node: the rows behind the last node are not written
    _, _, want_tok, want_status = infill_ref(s_in, tokens_in, s_model, drawn[:cells], region)
    got = raw(s_in, tokens_in, s_model, region, drawn, N=cells)
    assert got[0][:128 * G].tobytes() == want_s.astype(np.float32).tobytes() and got[1][:128 * G].tobytes() == want_s.astype(np.uint8).tobytes()
    assert np.array_equal(got[2][:G], want_forced) and got[5][:5].tolist() == want_status.tolist()
    assert np.array_equal(got[3][:30 * cells].reshape(-1, 15, 2), want_tok) and np.array_equal(got[3][30 * cells:30 * len(drawn)], drawn[cells:].reshape(-1))
    again = raw(s_in, tokens_in, s_model, region, drawn, N=cells)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    # N below the merged structure's cells: rows at and beyond N keep what they held, the counts still say what there is
    for N in (cells - 7, 1, 0):
        _, _, want_tok, want_status = infill_ref(s_in, tokens_in, s_model, drawn[:N], region)
        got = raw(s_in, tokens_in, s_model, region, drawn, N=N)
        assert np.array_equal(got[3][:30 * N].reshape(-1, 15, 2), want_tok) and np.array_equal(got[3][30 * N:30 * len(drawn)], drawn[N:].reshape(-1))
        assert got[5][:5].tolist() == want_status.tolist() and want_status[0] == cells and want_status[1] == N_in
    # N_in below the input's cells: the rows at and beyond it (poisoned here) are never read, their nodes have no source
    poisoned = tokens_in.copy()
    for n_in in (N_in - 11, 1, 0):
        poisoned[n_in:] = 7777
        _, _, want_tok, want_status = infill_ref(s_in, tokens_in[:n_in], s_model, drawn[:cells], region)
        got = raw(s_in, poisoned, s_model, region, drawn, N_in=n_in, N=cells)
        assert np.array_equal(got[3][:30 * cells].reshape(-1, 15, 2), want_tok) and not (got[3] == 7777).any()
        assert got[5][:5].tolist() == want_status.tolist() and want_status[0] == cells and want_status[1] == N_in and want_status[3] > 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------
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
    """the input: a generated NoteBatch (chord rules: every active cell holds a note), its bar graphs, its latent and its
    lists"""
    vae, zs, _ = model
    with _lib.deterministic(True), torch.no_grad():
        batch = generate_notes(vae, zs, chord_rules=ChordRules(), seed=3)[0]
        graph = batch.to_graph()
        mu, _ = encode_notes(vae, batch)
    return batch, graph, mu, batch.tolist()


def same_take(a, b):
    M = int(a[0].totals[0])
    return (torch.equal(a[0].totals, b[0].totals) and torch.equal(a[0].track_ptr, b[0].track_ptr)
            and torch.equal(a[0].notes[:M], b[0].notes[:M]) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])))


def node_tracks_and_bars(s_tensor):
    """(track, bar within the piece) of every node of a [B,n_bars,4,32] structure, in node order"""
    _, b, k, _ = np.nonzero(s_tensor.cpu().numpy())
    return k, b


def test_an_empty_region_returns_the_input(model, take):
    vae, _, n_bars = model
    batch, graph, mu, _ = take
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor, tokens, z, info = infill_notes(vae, batch, region_mask(n_bars, tracks=[]), temperature=0.9, seed=5,
                                                      return_tokens=True, return_z=True, return_info=True)
    M = int(batch.totals[0])
    assert torch.equal(out.track_ptr, batch.track_ptr) and torch.equal(out.notes[:M], batch.notes[:M]) and torch.equal(out.totals, batch.totals)
    assert s_tensor.dtype == torch.bool and torch.equal(s_tensor.reshape(-1, 4, 32).float(), graph.s_tensor)
    assert torch.equal(tokens, graph.tokens[:, 1:]) and torch.equal(z, mu)
    assert info.is_cuda and info.tolist() == [graph.num_nodes, graph.num_nodes, graph.num_nodes, 0, 0]
    assert out.n_bars == batch.n_bars and out.resolution == batch.resolution


def test_a_full_region_is_vary_notes_at_the_latent(model, take):
    vae, _, n_bars = model
    batch = take[0]
    kw = dict(temperature=0.9, return_tokens=True)
    with _lib.deterministic(True), torch.no_grad():
        for seed in (11, 12):
            assert same_take(infill_notes(vae, batch, region_mask(n_bars), seed=seed, **kw), vary_notes(vae, batch, strength=0, seed=seed, **kw))
        a = infill_notes(vae, batch, region_mask(n_bars), strength=1, seed=11, return_z=True, **kw)
        assert same_take(a[:3], vary_notes(vae, batch, strength=1, seed=11, **kw))


def test_two_tracks_regenerated_the_others_kept(model, take):
    vae, _, n_bars = model
    batch, graph, mu, lists = take
    region = region_mask(n_bars, tracks=["Guitar", "Strings"])
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor, tokens, info = infill_notes(vae, batch, region, temperature=0.9, seed=5, return_tokens=True, return_info=True)
        s_model = generate_notes(vae, mu)[1]
        s_in, tokens_in = graph.s_tensor.cpu().numpy(), graph.tokens.cpu().numpy()
        want_s, _, _, _ = infill_ref(s_in, tokens_in, s_model.cpu().numpy(), np.zeros((0, 15, 2)), region)
        assert np.array_equal(s_tensor.cpu().numpy().reshape(-1, 4, 32), want_s)
        # the draw, recomputed: the decoder on the merged structure's bar graphs, sample_tokens of its logits under the seed
        _, c_logits = vae.decoder(mu, vae.decoder._structure_from_binary(s_tensor.clone()))
        drawn = ops.sample_tokens(c_logits.detach().contiguous().float(), 0.9, None, None, 5)
    _, _, want_tokens, want_status = infill_ref(s_in, tokens_in, s_model.cpu().numpy(), drawn.cpu().numpy(), region)
    assert np.array_equal(tokens.cpu().numpy(), want_tokens) and info.tolist() == want_status.tolist()
    got = out.tolist()
    assert len(got) == len(lists) and all(g[:2] == w[:2] for g, w in zip(got, lists))
    assert any(g[2:] != w[2:] for g, w in zip(got, lists))


def test_one_bar_regenerated_the_others_kept(model, take):
    vae, _, n_bars = model
    batch, graph, _, lists = take
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor = infill_notes(vae, batch, region_mask(n_bars, bars=[1]), temperature=0.9, seed=6)
    outside = lambda piece: [[r for r in track if not 32 <= r[0] < 64] for track in piece]
    got = out.tolist()
    assert [outside(p) for p in got] == [outside(p) for p in lists] and got != lists
    assert torch.equal(s_tensor[:, 0].float(), graph.s_tensor.view(-1, n_bars, 4, 32)[:, 0])


def test_keep_structure_changes_only_the_notes_inside_the_region(model, take):
    vae, _, n_bars = model
    batch, graph, _, _ = take
    region = region_mask(n_bars, tracks=["Guitar"], bars=[0])
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor, tokens, info = infill_notes(vae, batch, region, keep_structure=True, temperature=0.9, seed=7, return_tokens=True,
                                                   return_info=True)
        with pytest.raises(ValueError, match="structure_rules draws the structure itself"):
            infill_notes(vae, batch, region, keep_structure=True, structure_rules=StructureRules(), seed=7)
    assert torch.equal(s_tensor.reshape(-1, 4, 32).float(), graph.s_tensor) and tokens.shape == (graph.num_nodes, 15, 2)
    track, bar = node_tracks_and_bars(s_tensor)
    inside = torch.from_numpy((track == 2) & (bar == 0)).to(DEV)
    changed = (tokens != graph.tokens[:, 1:]).any(-1).any(-1)
    assert inside.any() and not changed[~inside].any() and changed[inside].any()
    assert info.tolist() == [graph.num_nodes, graph.num_nodes, int((~inside).sum()), 0, 0]


def test_chord_rules_hold_in_the_regenerated_cells(model, take):
    vae, _, n_bars = model
    batch = take[0]
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor, tokens = infill_notes(vae, batch, region_mask(n_bars, tracks=["Guitar", "Strings"]), chord_rules=ChordRules(),
                                             temperature=0.9, seed=8, return_tokens=True)
    track, _ = node_tracks_and_bars(s_tensor)
    rows = tokens.cpu().numpy()[track >= 2]
    assert len(rows) > 0
    for row in rows:
        n = int(np.argmax(row[:, 0] == EOS[0]))
        assert row[n].tolist() == list(EOS) and 1 <= n <= 14 and (row[:n, 0] < 128).all() and len(set(row[:n, 0].tolist())) == n
        assert (row[n + 1:] == PAD).all() and (row[:n, 1] < 96).all()


def test_structure_rules_bound_the_regenerated_track(model, take):
    vae, _, n_bars = model
    batch, graph, _, _ = take
    with _lib.deterministic(True), torch.no_grad():
        out, s_tensor = infill_notes(vae, batch, region_mask(n_bars, tracks=["Strings"]), seed=9,
                                     structure_rules=StructureRules(max_active=(8, 4, 4, 2)))
    assert int(s_tensor[:, :, 3].sum(-1).max()) <= 2
    want = graph.s_tensor.view(-1, n_bars, 4, 32).bool().clone()
    want[:, :, 3] = s_tensor[:, :, 3]
    empty = ~want.any(-1).any(-1)
    want[..., 0, 0] |= empty                                             # (a bar that held Strings cells only)
    assert torch.equal(s_tensor, want)


def test_one_seed_one_take_and_the_status_adds_up(model, take):
    vae, _, n_bars = model
    batch, _, mu, _ = take
    region = region_mask(n_bars, tracks=["Bass", "Guitar"], steps=step_mask(lo=8, hi=23))
    kw = dict(temperature=0.9, strength=1, return_tokens=True, return_z=True, return_info=True)
    with _lib.deterministic(True), torch.no_grad():
        a, b, c = (infill_notes(vae, batch, region, seed=s, **kw) for s in (11, 11, 12))
    assert same_take(a, b) and not torch.equal(a[3], c[3]) and not torch.equal(a[3], mu)
    out, s_tensor, tokens, z, info = a
    cells, cells_in, kept, lost, forced = info.tolist()
    drawn = int((s_tensor & torch.from_numpy(region).to(DEV)).sum())
    assert cells == tokens.shape[0] == int(s_tensor.sum()) and kept + drawn == cells and lost <= forced
