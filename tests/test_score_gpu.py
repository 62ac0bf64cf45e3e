"""Per-piece scores on the device (csrc/score.hip; "Scores" in include/polyphemus_hip.h) against the float64 restatement of
tests/score_util.py, and `score_graph` / `score_notes` end to end.

The tolerance of the log-probabilities is measured, not fixed: the worst absolute error of torch's own float32
`log_softmax` + gather (tokens) and `binary_cross_entropy_with_logits` (structure) on the device against the float64
restatement, taken once over the rows (cells) of all the cases of this module; the kernels may be at most 4 x that per row
(per cell), and a sum of rows at most 4 x that times its number of rows.  The margin covers a different summation order over
131 / 99 terms and different expf / logf: both errors are a few ulp of log Z plus an ulp of |x_t - m|.
Measured on an MI355X (printed by the tests, kept in MEASURED below): torch 1.913e-06 per row, the kernel 1.913e-06 (one ulp
of a log-probability in [-32, -16)); torch 2.068e-07 per structure cell, the kernel 4.706e-07 on its worst sum of 32 cells."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import NoteBatch, NoteScores, score_graph, score_notes
from polyphemus_amd.model import VAE
from score_util import (N_PITCH, SLOTS, score_structure_ref, score_tokens_ref, structure_case, structure_terms_ref, structures,
                        targets_of, token_case)
from util import GOLDEN, REL_TOL, batch_from_golden, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0
# worst absolute error against float64 on an MI355X: (torch float32, the kernel)
MEASURED = {"row_logp": (1.913e-06, 1.913e-06), "structure_cell, sum of 32": (2.068e-07, 4.706e-07)}

TOKEN_CASES = [(name, slots) for name in structures() for slots in (15, 16)]
_cache = {}


def token_inputs(name, slots):
    """(x, t, s on the host, the restatement's outputs) of a case, computed once."""
    key = (name, slots)
    if key not in _cache:
        s = structures()[name]
        x, t = token_case(s, slots, seed=7)
        _cache[key] = (x, t, s, score_tokens_ref(x, t, s))
    return _cache[key]


def torch_row_error():
    """The worst absolute error of torch's float32 log_softmax + gather on the device over the rows of all TOKEN_CASES."""
    if "e_rows" not in _cache:
        worst = 0.0
        for name, slots in TOKEN_CASES:
            x, t, _, (_, _, row_logp, verdict) = token_inputs(name, slots)
            xd, tgt = torch.from_numpy(x).to(DEV), torch.from_numpy(targets_of(t).astype(np.int64)).to(DEV)
            for h, (lo, hi, bit) in enumerate(((0, N_PITCH, 4), (N_PITCH, 230, 8))):
                on = torch.from_numpy((verdict & bit) != 0).to(DEV)
                lp = F.log_softmax(xd[..., lo:hi], dim=-1).gather(-1, torch.where(on, tgt[..., h], 0)[..., None])[..., 0]
                err = (lp.double().cpu().numpy() - row_logp[..., h])[on.cpu().numpy()]
                worst = max(worst, float(np.abs(err).max()))
        _cache["e_rows"] = worst
    return _cache["e_rows"]


def as_bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(as_bits(a), as_bits(b))


@pytest.mark.parametrize("name,slots", TOKEN_CASES)
def test_score_tokens_matches_the_restatement(name, slots):
    x, t, s, (logp_ref, counts_ref, row_ref, verdict_ref) = token_inputs(name, slots)
    e_torch = torch_row_error()
    logp, counts, row_logp, verdict = ops.score_tokens(torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV),
                                                       torch.from_numpy(s).to(DEV), return_verdict=True)
    assert logp.shape == s.shape[:2] + (4, 2) and logp.dtype == torch.float64
    assert counts.shape == s.shape[:2] + (4, 6) and counts.dtype == torch.int32
    assert row_logp.shape == (x.shape[0], SLOTS, 2) and row_logp.dtype == torch.float32 and verdict.dtype == torch.uint8
    assert np.array_equal(verdict.cpu().numpy(), verdict_ref)
    assert np.array_equal(counts.cpu().numpy().reshape(counts_ref.shape), counts_ref)
    err = np.abs(row_logp.double().cpu().numpy() - row_ref)
    print(f"\n[score_tokens {name} tok_slots={slots}] torch fp32 worst row error {e_torch:.3e}, kernel {err.max():.3e}")
    assert np.isfinite(row_logp.cpu().numpy()).all() and e_torch > 0
    assert (row_logp.cpu().numpy()[(verdict_ref[..., None] & np.array([4, 8])) == 0] == 0).all()          # a PAD target: exactly 0
    assert err.max() <= MARGIN * e_torch, (err.max(), e_torch)
    rows = counts_ref[..., 1:3].astype(np.float64)                                                         # rows behind each sum
    err_sum = np.abs(logp.cpu().numpy().reshape(logp_ref.shape) - logp_ref)
    assert (err_sum <= MARGIN * e_torch * rows).all(), (err_sum.max(), e_torch)


def _raw_tokens(x, t, s, N):
    """pm_score_tokens through the raw binding on buffers filled with sentinels and followed by 64 sentinel words."""
    G, TAIL = s.reshape(-1, 128).shape[0], 64
    xd, td, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(s.astype(np.float32)).to(DEV)
    NAN32, NAN64 = 0x7FC12345, 0x7FF8123456789ABC
    bufs = dict(bar_nodes=torch.full((G + TAIL,), -77, dtype=torch.int32, device=DEV),
                node_ptr=torch.full((G + 1 + TAIL,), -77, dtype=torch.int32, device=DEV),
                row_logp=torch.full((N * 30 + TAIL,), NAN32, dtype=torch.int32, device=DEV),
                verdict=torch.full((N * 15 + TAIL,), 0xEE, dtype=torch.uint8, device=DEV),
                logp=torch.full((G * 8 + TAIL,), NAN64, dtype=torch.int64, device=DEV),
                counts=torch.full((G * 24 + TAIL,), -77, dtype=torch.int32, device=DEV))
    sent = dict(bar_nodes=-77, node_ptr=-77, row_logp=NAN32, verdict=0xEE, logp=NAN64, counts=-77)
    rc = _lib.lib().pm_score_tokens(xd.data_ptr(), td.data_ptr(), t.shape[1], sd.data_ptr(), G, N, bufs["bar_nodes"].data_ptr(),
                                    bufs["node_ptr"].data_ptr(), bufs["row_logp"].data_ptr(), bufs["verdict"].data_ptr(),
                                    bufs["logp"].data_ptr(), bufs["counts"].data_ptr(), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        body, tail = b[:-TAIL], b[-TAIL:]
        assert not (body == sent[k]).any(), f"{k}: a word was not written"
        assert (tail == sent[k]).all(), f"{k}: written behind the buffer"
        out[k] = body
    return (out["logp"].view(torch.float64).view(G, 4, 2), out["counts"].view(G, 4, 6), out["row_logp"].view(torch.float32).view(N, 15, 2),
            out["verdict"].view(N, 15), out["node_ptr"])


@pytest.mark.parametrize("slots", [15, 16])
def test_raw_binding_writes_every_word_and_nothing_behind(slots):
    x, t, s, (logp_ref, counts_ref, row_ref, verdict_ref) = token_inputs("three_bars", slots)
    N = x.shape[0]
    e_torch = torch_row_error()
    logp, counts, row_logp, verdict, node_ptr = _raw_tokens(x, t, s, N)
    assert int(node_ptr[-1]) == N
    assert np.array_equal(counts.cpu().numpy(), counts_ref) and np.array_equal(verdict.cpu().numpy(), verdict_ref)
    assert np.abs(row_logp.double().cpu().numpy() - row_ref).max() <= MARGIN * e_torch
    assert (counts[1, 2] == 0).all() and (logp[1, 2] == 0).all()                        # the empty track: zeros, written
    # fewer rows than the structure has active cells: the nodes at N and beyond are ignored, node_ptr[G] still counts them
    M = N - 37
    part_ref = score_tokens_ref(x[:M], t[:M], s, N=M)
    logp, counts, row_logp, verdict, node_ptr = _raw_tokens(x[:M].copy(), t[:M].copy(), s, M)
    assert int(node_ptr[-1]) == N and int(counts[..., 0].sum()) == M
    assert np.array_equal(counts.cpu().numpy(), part_ref[1]) and np.array_equal(verdict.cpu().numpy(), part_ref[3])
    assert (np.abs(logp.cpu().numpy() - part_ref[0]) <= MARGIN * e_torch * part_ref[1][..., 1:3]).all()

    # pm_score_structure the same way
    G, TAIL = 3, 64
    xs, ys = structure_case(G, seed=11)
    lp = torch.full((G * 4 + TAIL,), 0x7FF8123456789ABC, dtype=torch.int64, device=DEV)
    cn = torch.full((G * 16 + TAIL,), -77, dtype=torch.int32, device=DEV)
    xd, yd = torch.from_numpy(xs).to(DEV), torch.from_numpy(ys.astype(np.float32)).to(DEV)
    assert _lib.lib().pm_score_structure(xd.data_ptr(), yd.data_ptr(), G, lp.data_ptr(), cn.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert not (lp[:-TAIL] == 0x7FF8123456789ABC).any() and (lp[-TAIL:] == 0x7FF8123456789ABC).all()
    assert (cn[-TAIL:] == -77).all() and np.array_equal(cn[:-TAIL].view(G, 4, 4).cpu().numpy(), score_structure_ref(xs, ys)[1])


def test_scores_are_reproducible_and_independent_of_the_rest_of_the_batch():
    x, t, s, _ = token_inputs("two_pieces", 16)
    xd, td, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV), torch.from_numpy(s).to(DEV)
    first = ops.score_tokens(xd, td, sd, return_verdict=True)
    again = ops.score_tokens(xd, td, sd, return_verdict=True)
    assert all(same_bits(a, b) for a, b in zip(first, again))
    na = int(s[0].sum())
    assert 0 < na < x.shape[0]
    alone = [ops.score_tokens(xd[lo:hi].contiguous(), td[lo:hi].contiguous(), sd[i:i + 1], return_verdict=True)
             for i, (lo, hi) in enumerate(((0, na), (na, x.shape[0])))]
    for k in range(4):
        assert same_bits(first[k], torch.cat([alone[0][k], alone[1][k]])), k
    xs, ys = structure_case(3, seed=11)
    xs, ys = torch.from_numpy(xs).to(DEV), torch.from_numpy(ys).to(DEV)
    a, b = ops.score_structure(xs, ys), ops.score_structure(xs, ys)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    for g in range(3):                                                                   # a bar alone (its half-wave's other half empty)
        one = ops.score_structure(xs[:, g:g + 1].contiguous(), ys[:, g:g + 1].contiguous())
        assert same_bits(one[0], a[0][:, g:g + 1].contiguous()) and same_bits(one[1], a[1][:, g:g + 1].contiguous())


@pytest.mark.parametrize("G", [1, 3])
def test_score_structure_matches_the_restatement(G):
    x, y = structure_case(G, seed=11)
    logp_ref, counts_ref = score_structure_ref(x, y)
    xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    # torch's own float32 BCE with logits on the device, per cell, over the cells of both cases of this test
    if "e_cells" not in _cache:
        worst = 0.0
        for g in (1, 3):
            xg, yg = structure_case(g, seed=11)
            got = F.binary_cross_entropy_with_logits(torch.from_numpy(xg).to(DEV), torch.from_numpy(yg).float().to(DEV), reduction="none")
            worst = max(worst, float(np.abs(got.double().cpu().numpy().reshape(-1, 4, 32) - structure_terms_ref(xg, yg)).max()))
        _cache["e_cells"] = worst
    e_torch = _cache["e_cells"]
    logp, counts = ops.score_structure(xd, yd)
    assert logp.shape == (1, G, 4) and logp.dtype == torch.float64 and counts.shape == (1, G, 4, 4) and counts.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy()[0], counts_ref)
    err = np.abs(logp.cpu().numpy()[0] - logp_ref)
    print(f"\n[score_structure G={G}] torch fp32 worst cell error {e_torch:.3e}, kernel worst 32-cell sum error {err.max():.3e}")
    assert np.isfinite(logp.cpu().numpy()).all() and e_torch > 0
    assert err.max() <= MARGIN * e_torch * 32, (err.max(), e_torch)
    # any dtype of the structure
    for alt in (yd.float(), yd.to(torch.uint8), yd.double()):
        got = ops.score_structure(xd, alt)
        assert same_bits(got[0], logp) and same_bits(got[1], counts)


def _golden_model(case="lmd2_tiny"):
    z, cfg = load_case(case)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    return z, cfg, vae


def test_score_graph_reproduces_the_reference_metrics_of_the_golden_case():
    """`score_graph` at the reference's latent (mu + exp(log_var / 2) eps, the golden eps) against what the reference's
    `evaluate` recorded for the same batch (tests/golden/lmd2_tiny_metrics.npz): the two cross-entropies are the summed
    log-probabilities over the targets, the five content accuracies the summed hits over theirs.  The structure scores are
    compared with the float64 BCE of the decoder's own structure logits, not with the recorded 'structure' loss, which the
    reference takes on the target itself (quirk B-1).  Deterministic mode: the decoder then gives the same logits to the
    test and to `score_graph`."""
    z, cfg, vae = _golden_model()
    m = np.load(os.path.join(GOLDEN, "lmd2_tiny_metrics.npz"), allow_pickle=True)
    losses, accs = json.loads(str(m["losses"])), json.loads(str(m["accs"]))
    g = batch_from_golden(z, cfg).to(DEV)
    eps = torch.from_numpy(z["in/eps"]).to(DEV)
    vae.train()
    with _lib.deterministic(True):
        at_mu = score_graph(vae, g)
        assert vae.training and at_mu.z.shape == (1,) + tuple(at_mu.mu.shape) and torch.equal(at_mu.z[0], at_mu.mu)
        zz = at_mu.mu + torch.exp(0.5 * at_mu.log_var) * eps
        sc = score_graph(vae, g, z=zz)
        vae.eval()
        with torch.no_grad():
            s_logits, c_logits = vae.decoder(zz, g)
        vae.train()
    assert isinstance(sc, NoteScores) and vae.training
    B, nb = g.s_tensor.shape[0] // cfg["n_bars"], cfg["n_bars"]
    assert sc.content_logp.shape == (1, B, nb, 4, 2) and sc.content_counts.shape == (1, B, nb, 4, 6)
    assert sc.structure_logp.shape == (1, B, nb, 4) and sc.structure_counts.shape == (1, B, nb, 4, 4)
    assert len(sc.row_logp) == 1 and sc.row_logp[0].shape == (g.tokens.shape[0], 15, 2)
    c = sc.content_counts.double().sum(dim=(0, 1, 2)).cpu().numpy()                       # [4,6]
    lp = sc.content_logp.sum(dim=(0, 1, 2, 3)).cpu().numpy()
    assert int(c[:, 0].sum()) == g.tokens.shape[0]
    got = {"pitch": -lp[0] / c[:, 1].sum(), "dur": -lp[1] / c[:, 2].sum()}
    for k, v in got.items():
        print(f"\n[golden] loss {k}: {v!r} reference {losses[k]!r}")
        assert abs(v - losses[k]) <= REL_TOL * max(1.0, abs(losses[k])), (k, v, losses[k])
    got = {"pitch": c[:, 3].sum() / c[:, 1].sum(), "dur": c[:, 4].sum() / c[:, 2].sum(), "note": c[:, 5].sum() / c[:, 1].sum(),
           "pitch_drums": c[0, 3] / c[0, 1], "pitch_non_drums": c[1:, 3].sum() / c[1:, 1].sum()}
    for k, v in got.items():
        assert abs(v - accs[k]) < 1e-6, (k, v, accs[k])
    # the same numbers from the per-piece methods, weighted back by their denominators
    a = sc.accuracies()
    tp = sc.content_counts[..., 1].sum(dim=(2, 3)).double()
    assert abs(float((a["pitch"] * tp).sum() / tp.sum()) - accs["pitch"]) < 1e-6
    assert torch.allclose(sc.log_likelihood(structure=False), sc.per_bar().sum(-1) - sc.structure_logp.sum(dim=(2, 3)))
    assert torch.allclose(sc.log_likelihood(), sc.per_track().sum(-1))
    # structure: the float64 BCE of the decoder's own logits
    s_ref, sc_ref = score_structure_ref(s_logits.float().cpu().numpy(), g.s_tensor.cpu().numpy())
    assert np.array_equal(sc.structure_counts[0].cpu().numpy().reshape(sc_ref.shape), sc_ref)
    got_s = sc.structure_logp[0].cpu().numpy().reshape(s_ref.shape)
    assert (np.abs(got_s - s_ref) <= REL_TOL * np.maximum(1.0, np.abs(s_ref))).all()
    # and the tokens against the restatement on the decoder's own logits
    t_ref = score_tokens_ref(c_logits.float().cpu().numpy(), g.tokens.cpu().numpy(), g.s_tensor.cpu().numpy())
    assert np.array_equal(sc.content_counts[0].cpu().numpy().reshape(t_ref[1].shape), t_ref[1])
    assert (np.abs(sc.content_logp[0].cpu().numpy().reshape(t_ref[0].shape) - t_ref[0]) <= REL_TOL * np.maximum(1.0, np.abs(t_ref[0]))).all()


def test_score_notes_equals_score_graph_and_its_samples_are_reproducible():
    """Deterministic mode, so that two decoder passes on the same latent give the same logits bit for bit."""
    _, cfg, vae = _golden_model()
    nb = cfg["n_bars"]
    pieces = [[[(0, 36, 2), (8, 38, 2), (16, 36, 2), (24, 38, 2), (32 * (nb - 1) + 4, 42, 1)], [(0, 40, 8), (16, 43, 8)],
               [(0, 60, 4), (0, 64, 4), (0, 67, 4), (32 * (nb - 1), 62, 16)], []],
              [[(4, 36, 1)], [], [(32 * (nb - 1) + 31, 72, 9)], [(0, 48, 32), (0, 55, 32)]]]
    batch = NoteBatch.from_lists(pieces, nb, device=DEV)
    vae.train()
    with _lib.deterministic(True):
        a = score_notes(vae, batch)
        assert vae.training
        b = score_graph(vae, batch.to_graph())
        fields = ("content_logp", "content_counts", "structure_logp", "structure_counts", "mu", "log_var", "z")
        assert all(same_bits(getattr(a, f), getattr(b, f)) for f in fields) and same_bits(a.row_logp[0], b.row_logp[0])
        assert torch.equal(a.z[0], a.mu) and int(a.content_counts[..., 0].sum()) == a.row_logp[0].shape[0]
        s3 = score_notes(vae, batch, samples=3, seed=99)
        again = score_notes(vae, batch, samples=3, seed=99)
        other = score_notes(vae, batch, samples=3, seed=100)
        assert all(same_bits(getattr(s3, f), getattr(again, f)) for f in fields) and not torch.equal(s3.z, other.z)
        assert s3.z.shape == (3,) + tuple(s3.mu.shape) and s3.content_logp.shape[0] == 3 and len(s3.row_logp) == 3
        eps = torch.randn((3,) + tuple(s3.mu.shape), generator=torch.Generator().manual_seed(99), dtype=torch.float32).to(DEV)
        assert torch.equal(s3.z, s3.mu[None] + torch.exp(0.5 * s3.log_var)[None] * eps)
        for k in range(3):
            one = score_notes(vae, batch, z=s3.z[k])
            for f in fields[:4]:
                assert same_bits(getattr(one, f)[0], getattr(s3, f)[k]), (k, f)
            assert same_bits(one.row_logp[0], s3.row_logp[k])
        full = score_notes(vae, batch, z=s3.z)
        assert all(same_bits(getattr(full, f), getattr(s3, f)) for f in fields)
        seeded = score_notes(vae, batch, seed=99)                                          # a seed alone draws one latent
        assert seeded.z.shape[0] == 1 and not torch.equal(seeded.z[0], seeded.mu)
        vae.eval()
        assert not score_notes(vae, batch).content_logp.requires_grad and not vae.training
    # ELBO and the importance-weighted bound from the returned fields
    mu, lv, zk = s3.mu.double().cpu(), s3.log_var.double().cpu(), s3.z.double().cpu()
    ll = (s3.content_logp.sum(dim=(2, 3, 4)) + s3.structure_logp.sum(dim=(2, 3))).cpu()
    kl = -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(1)
    assert torch.allclose(s3.kl().cpu(), kl, rtol=1e-12, atol=0) and (kl > 0).all()
    assert torch.allclose(s3.elbo().cpu(), ll - kl[None], rtol=1e-12, atol=1e-9)
    assert torch.allclose(s3.elbo(beta=0.25).cpu(), ll - 0.25 * kl[None], rtol=1e-12, atol=1e-9)
    log_prior = torch.distributions.Normal(0.0, 1.0).log_prob(zk).sum(-1)
    log_q = torch.distributions.Normal(mu, (0.5 * lv).exp()).log_prob(zk).sum(-1)
    want = torch.logsumexp(ll + log_prior - log_q, dim=0) - np.log(3.0)
    assert torch.allclose(s3.iwae().cpu(), want, rtol=1e-10, atol=1e-8)
    n_tok = s3.content_counts[..., 1:3].sum(dim=(2, 3, 4)).double().cpu()
    assert torch.allclose(s3.nll_per_token().cpu(), -s3.content_logp.sum(dim=(2, 3, 4)).cpu() / n_tok)
    assert torch.allclose(s3.perplexity().cpu(), torch.exp(s3.nll_per_token().cpu()))
    acc = s3.accuracies()
    assert set(acc) == {"pitch", "dur", "note", "pitch_drums", "pitch_non_drums", "s_precision", "s_recall", "s_f1"}
    assert all(v.shape == (3, 2) for v in acc.values())
