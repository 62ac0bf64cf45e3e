"""Sampled generation on the device (csrc/sample.hip, k_mtp_fill<true> of csrc/generate.hip, generate_music's sampling
arguments) against an fp64 numpy restatement of the definition in include/polyphemus_hip.h ("sampled generation"), the
binomial bounds of the distribution it must draw from, and the oracle's pianoroll layout."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import vae_cpu
from polyphemus_amd import _lib, ops
from polyphemus_amd.generate import generate_music
from polyphemus_amd.model import VAE
from test_sampling_abi import sample_hash_np
from util import GOLDEN, load_case, state_dict_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
HEADS = ((0, 131), (131, 230))
OFF = None
CONFIGS = [(1.0, OFF, OFF), (0.5, 5, OFF), (1.5, OFF, 0.9), (1.0, 40, 0.9)]        # (temperature, top_k, top_p)
SCORE_GAP, MASS_EDGE, LEFT_OUT_CAP = 1e-3, 1e-5, 0.02


def replica(logits, temperature, top_k, top_p, seed):
    """The definition, in fp64 on the fp32 logits [R,230]: (tokens [R,2], decided [R,2]).  A (row, head) is not decided
    when its two best scores are closer than SCORE_GAP or some token's outranking mass is within MASS_EDGE * Z of the
    nucleus edge top_p * Z: there fp32 may honestly choose otherwise."""
    R = logits.shape[0]
    inv_t = float(np.float32(1.0 / temperature)) if temperature > 0 else None
    tokens, decided = np.zeros((R, 2), np.int64), np.ones((R, 2), bool)
    rows = np.arange(R, dtype=np.uint64)[:, None]
    for head, (c0, c1) in enumerate(HEADS):
        l = logits[:, c0:c1].astype(np.float64)
        V = c1 - c0
        order = np.argsort(-l, axis=1, kind="stable")                              # equal logits: lower index first
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.broadcast_to(np.arange(V), order.shape), axis=1)
        if temperature == 0:
            tokens[:, head] = order[:, 0]
            continue
        live = rank < top_k if top_k is not None and 0 < top_k < V else np.ones_like(l, bool)
        if top_p is not None and top_p < 1:
            q = np.where(live, np.exp((l - l.max(1, keepdims=True)) * inv_t), 0.0)
            qs = np.take_along_axis(q, order, axis=1)
            before = np.empty_like(q)
            np.put_along_axis(before, order, np.cumsum(qs, axis=1) - qs, axis=1)   # mass of the survivors that outrank it
            Z = q.sum(1, keepdims=True)
            edge = float(np.float32(top_p)) * Z
            decided[:, head] &= ~(live & (np.abs(before - edge) < MASS_EDGE * Z)).any(1)
            live &= before < edge
        u = (sample_hash_np(seed, rows, head, np.arange(V, dtype=np.uint64)[None, :]).astype(np.float64) + 0.5) / (1 << 23)
        score = np.where(live, l * inv_t - np.log(-np.log(u)), -np.inf)
        tokens[:, head] = score.argmax(1)                                          # numpy: the first of equal maxima
        top2 = np.sort(score, axis=1)[:, -2:]
        decided[:, head] &= ~(top2[:, 1] - top2[:, 0] < SCORE_GAP)
    return tokens, decided


def _check_against_replica(logits, T, k, p, seed, what):
    got = ops.sample_tokens(logits.to(DEV), T, k, p, seed).cpu().numpy()
    assert got.shape == (logits.shape[0], 15, 2) and got.dtype == np.int32
    want, decided = replica(logits.reshape(-1, 230).numpy(), T, k, p, seed)
    got = got.reshape(-1, 2)
    left_out = 1.0 - decided.mean()
    print(f"{what}: {decided.size} pairs, {left_out:.4f} left out, {(got != want)[decided].sum()} decided pairs differ")
    assert left_out <= LEFT_OUT_CAP, (what, left_out)
    assert np.array_equal(got[decided], want[decided]), (what, np.argwhere((got != want) & decided)[:8])
    assert got.min() >= 0 and (got[:, 0] < 131).all() and (got[:, 1] < 99).all()


@pytest.mark.parametrize("N", [1, 5, 273])
def test_sampled_tokens_equal_the_fp64_replica(N):
    """A case is one (N, scale, configuration).  The replica alone leaves out about 0.5 % of the pairs of a nucleus case;
    a case of N = 1 has 30 pairs, so a single pair left out is over the cap: the generator seeds are ones at which the
    replica (nothing of the device enters that) leaves none out there."""
    for scale in (1, 3):
        logits = torch.randn(N, 15, 230, generator=torch.Generator().manual_seed(2000 + 100 * N + scale)) * scale
        for i, (T, k, p) in enumerate(CONFIGS):
            _check_against_replica(logits, T, k, p, 1000 + i, (N, scale, T, k, p))


def test_sampled_tokens_rank_equal_logits_by_index():
    """Logits on a grid of 0.5: every row has runs of equal logits across the top-k and the nucleus edges, which the
    definition breaks by the lower index (the replica's stable sort)."""
    logits = (torch.randn(5, 15, 230, generator=torch.Generator().manual_seed(9)) * 2).round() / 2
    for i, (T, k, p) in enumerate([(1.0, 5, OFF), (1.0, 40, OFF), (0.7, 98, OFF), (1.0, OFF, 0.5), (1.0, 40, 0.9)]):
        got = ops.sample_tokens(logits.to(DEV), T, k, p, 50 + i).cpu().numpy().reshape(-1, 2)
        want, decided = replica(logits.reshape(-1, 230).numpy(), T, k, p, 50 + i)
        assert decided.mean() > 0.5 and np.array_equal(got[decided], want[decided]), (T, k, p)


def test_greedy_is_the_argmax_and_top_k_1_at_any_temperature():
    logits = torch.randn(273, 15, 230, generator=torch.Generator().manual_seed(4)) * 3
    logits[0, 0, 7] = logits[0, 0, 100] = 50.0                    # two equal maxima: the lower index
    logits[0, 0, 131 + 98] = logits[0, 0, 131 + 3] = 50.0
    logits[1, 14, 130] = logits[1, 14, 0] = logits[1, 14, 64] = 60.0
    logits[2, 3, :] = 0.25                                        # a constant row: token 0 of both heads
    logits[3, 3, :131] = -0.0
    logits[3, 3, 5] = 0.0                                         # -0 == +0: still token 0
    x = logits.to(DEV)
    greedy = ops.sample_tokens(x, temperature=0)
    want = np.stack([logits[..., :131].numpy().argmax(-1), logits[..., 131:].numpy().argmax(-1)], -1)
    assert np.array_equal(greedy.cpu().numpy(), want)
    assert tuple(want[0, 0]) == (7, 3) and tuple(want[1, 14])[0] == 0 and tuple(want[2, 3]) == (0, 0) and want[3, 3, 0] == 0
    for kw in (dict(temperature=1.0, top_k=1), dict(temperature=0.3, top_k=1, seed=9), dict(temperature=5.0, top_k=1, top_p=0.5),
               dict(temperature=0, top_k=7, top_p=0.4, seed=3)):
        assert torch.equal(ops.sample_tokens(x, **kw), greedy), kw
    dev = torch.stack([x[..., :131].argmax(-1), x[..., 131:].argmax(-1)], -1)
    untied = torch.ones(273, 15, dtype=torch.bool)
    untied[0, 0] = untied[1, 14] = untied[2, 3] = untied[3, 3] = False
    assert torch.equal(greedy.cpu()[untied].long(), dev.cpu()[untied])


# ---- the distribution: R identical rows, a known four-point law per head --------------------------------------------
R_DIST, N_DIST = 65550, 4370
P_PITCH = {0: 0.5, 63: 0.25, 64: 0.15, 130: 0.1}
P_DUR = {0: 0.4, 63: 0.3, 64: 0.2, 98: 0.1}


@pytest.fixture(scope="module")
def dist_logits():
    row = torch.full((230,), -30.0)
    for t, p in P_PITCH.items():
        row[t] = float(np.log(p))
    for t, p in P_DUR.items():
        row[131 + t] = float(np.log(p))
    assert N_DIST * 15 == R_DIST
    return row.expand(N_DIST, 15, 230).contiguous().to(DEV), row.double().numpy()


def _bound(p):
    return 5.0 * (p * (1.0 - p) / R_DIST) ** 0.5


def _shares(tokens, head, V):
    return np.bincount(tokens.reshape(-1, 2)[:, head], minlength=V) / R_DIST


def _check_shares(tokens, head, expect, named, what):
    """every named token's share, and the share of all the other tokens together, within the binomial bound of `expect`"""
    got = _shares(tokens, head, len(expect))
    rest = np.ones(len(expect), bool)
    rest[list(named)] = False
    pairs = [(f"token {t}", got[t], expect[t]) for t in named] + [("the other tokens", got[rest].sum(), expect[rest].sum())]
    for name, g, e in pairs:
        print(f"{what} head {head} {name}: share {g:.6f}, expected {e:.6f} +- {_bound(e):.6f}")
    for name, g, e in pairs:
        assert abs(g - e) <= _bound(e), (what, head, name, g, e)


def _softmax(l):
    e = np.exp(l - l.max())
    return e / e.sum()


def test_sampled_shares_follow_the_distribution(dist_logits):
    x, row = dist_logits
    lp, ld = row[:131], row[131:]
    t1 = ops.sample_tokens(x, seed=11).cpu().numpy()
    _check_shares(t1, 0, _softmax(lp), P_PITCH, "T=1")
    _check_shares(t1, 1, _softmax(ld), P_DUR, "T=1")
    for t, p in P_PITCH.items():                                   # (fp32 log p and the -30 floor move the four shares by 1e-8)
        assert abs(_softmax(lp)[t] - p) < 1e-7
    t2 = ops.sample_tokens(x, temperature=2.0, seed=12).cpu().numpy()
    _check_shares(t2, 0, _softmax(lp / 2), P_PITCH, "T=2")           # proportional to sqrt(p)
    _check_shares(t2, 1, _softmax(ld / 2), P_DUR, "T=2")
    two = lambda V, a, b, wa, wb: np.bincount([a, b], weights=[wa, wb], minlength=V)
    tk = ops.sample_tokens(x, top_k=2, seed=13).cpu().numpy()     # the two best tokens survive, every other share is 0
    _check_shares(tk, 0, two(131, 0, 63, 2 / 3, 1 / 3), P_PITCH, "top_k=2")
    _check_shares(tk, 1, two(99, 0, 63, 4 / 7, 3 / 7), P_DUR, "top_k=2")
    # top_p = 0.7 leaves the same two pitch tokens (outranking masses 0, 0.5 | 0.75, 0.9 against the edge 0.7).  The duration
    # head's third token has the outranking mass 0.4 + 0.3, on the edge itself: undecided by definition, so only its first
    # two tokens (masses 0, 0.4) and its last (0.9) are pinned: 0 and 63 keep the ratio 4 : 3, 98 never comes out
    tn = ops.sample_tokens(x, top_p=0.7, seed=13).cpu().numpy()
    _check_shares(tn, 0, two(131, 0, 63, 2 / 3, 1 / 3), P_PITCH, "top_p=0.7")
    d = _shares(tn, 1, 99)
    assert d[98] == 0 and d[0] + d[63] + d[64] == 1.0
    n2 = (d[0] + d[63]) * R_DIST
    assert abs(d[0] * R_DIST / n2 - 4 / 7) <= 5.0 * ((4 / 7) * (3 / 7) / n2) ** 0.5
    # the heads are independent: the joint share is the product of the marginals
    a, b = t1.reshape(-1, 2)[:, 0], t1.reshape(-1, 2)[:, 1]
    for tp, pp in P_PITCH.items():
        for td, pd in P_DUR.items():
            joint = float(((a == tp) & (b == td)).mean())
            assert abs(joint - pp * pd) <= _bound(pp * pd), (tp, td, joint, pp * pd)
    # two seeds agree on a row with probability sum p^2; one seed agrees with itself everywhere
    other = ops.sample_tokens(x, seed=14).cpu().numpy()
    for head, law in ((0, P_PITCH), (1, P_DUR)):
        same = float((t1[..., head] == other[..., head]).mean())
        p2 = sum(p * p for p in law.values())
        assert abs(same - p2) <= _bound(p2), (head, same, p2)
    assert np.array_equal(ops.sample_tokens(x, seed=11).cpu().numpy(), t1)
    assert np.array_equal(ops.sample_tokens(x, top_k=2, seed=13).cpu().numpy(), ops.sample_tokens(x, top_k=2, seed=13).cpu().numpy())


def test_non_finite_logits_give_tokens_in_range_and_touch_nothing_else():
    N, pad, canary = 3, 3, -123456789
    logits = torch.randn(N, 15, 230, generator=torch.Generator().manual_seed(2))
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
    x = logits.to(DEV)
    rows = N * 15
    for kw in (dict(temperature=0.0), dict(temperature=1.0), dict(temperature=1e-30), dict(temperature=1e30),
               dict(temperature=0.5, top_k=5), dict(temperature=1.5, top_p=0.9), dict(temperature=1.0, top_k=40, top_p=0.9)):
        buf = torch.full((pad + rows * 2 + pad,), canary, dtype=torch.int32, device=DEV)
        _lib.call("pm_sample_tokens", x.data_ptr(), rows, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), 21,
                  buf.data_ptr() + 4 * pad, _lib.stream())
        out = buf.cpu().numpy()
        assert (out[:pad] == canary).all() and (out[-pad:] == canary).all(), kw
        tok = out[pad:-pad].reshape(rows, 2)
        assert tok.min() >= 0 and (tok[:, 0] < 131).all() and (tok[:, 1] < 99).all(), kw
    assert ops.sample_tokens(x[:0].contiguous()).shape == (0, 15, 2)


# ---- the pianoroll of the tokens ------------------------------------------------------------------------------------
def _one_hot(tokens):
    """float32 [N,15,230] with 1.0 at `pitch` and at 131 + `duration` where the token is inside its head's range."""
    N = tokens.shape[0]
    out = torch.zeros(N, 15, 230)
    tp, td = tokens[..., 0].long(), tokens[..., 1].long()
    okp, okd = (tp >= 0) & (tp < 131), (td >= 0) & (td < 99)
    out.scatter_(2, tp.clamp(0, 130).unsqueeze(-1), okp.float().unsqueeze(-1))
    out.scatter_(2, (131 + td.clamp(0, 98)).unsqueeze(-1), okd.float().unsqueeze(-1))
    return out


@pytest.mark.parametrize("G,p", [(1, 0.0), (1, 1.0), (5, 0.3), (64, 0.02), (33, 0.97)])
def test_mtp_from_tokens_matches_oracle(G, p):
    gen = torch.Generator().manual_seed(G)
    s = (torch.rand(1, G, 4, 32, generator=gen) < p)
    N = int(s.sum())
    tokens = torch.stack([torch.randint(0, 131, (N, 15), generator=gen), torch.randint(0, 99, (N, 15), generator=gen)], -1).int()
    if N:
        tokens[0, 0] = torch.tensor([130, 98])
        tokens[-1, 14] = torch.tensor([0, 0])
    got = ops.mtp_from_tokens(tokens.to(DEV), s.to(DEV)).cpu()
    assert torch.equal(got, vae_cpu.mtp_from_logits(_one_hot(tokens), s))
    if N:
        act = got[s]
        assert torch.equal(act[..., :131].argmax(-1).int(), tokens[..., 0]) and torch.equal(act[..., 131:].argmax(-1).int(), tokens[..., 1])


def test_mtp_from_tokens_raises_like_mtp_from_logits_and_skips_tokens_out_of_range():
    gen = torch.Generator().manual_seed(8)
    s = (torch.rand(2, 2, 4, 32, generator=gen) < 0.3).to(DEV)
    N = int(s.sum())
    tokens = torch.stack([torch.randint(0, 131, (N, 15), generator=gen), torch.randint(0, 99, (N, 15), generator=gen)], -1).int()
    for t, ss in ((tokens[:-1], s), (tokens[:, :14], s), (tokens, s[0]), (tokens, s[..., :31])):
        with pytest.raises(ValueError):
            ops.mtp_from_tokens(t.contiguous().to(DEV), ss)
        with pytest.raises(ValueError):
            ops.mtp_from_logits(torch.zeros(t.shape[0], t.shape[1], 230, device=DEV), ss)
    with pytest.raises(TypeError):
        ops.mtp_from_tokens(tokens.long().to(DEV), s)
    ops.mtp_from_tokens(tokens[:-1].contiguous().to(DEV), s, check=False)        # as mtp_from_logits: the caller's risk
    bad = tokens.clone()
    bad[0, 0] = torch.tensor([-1, 99])
    bad[0, 1] = torch.tensor([131, -1])
    bad[1, 2] = torch.tensor([2 ** 31 - 1, -2 ** 31])
    bad[N - 1, 14] = torch.tensor([-2 ** 31, 2 ** 31 - 1])
    bad[2, 3] = torch.tensor([230, 3])                                           # a pitch that would land in the duration head
    bad[2, 4] = torch.tensor([5, 99 + 131])
    got = ops.mtp_from_tokens(bad.to(DEV), s).cpu()
    assert torch.equal(got, vae_cpu.mtp_from_logits(_one_hot(bad), s.cpu()))
    act = got[s.cpu()]
    assert float(act[0, 0].sum()) == 0 and float(act[0, 1].sum()) == 0 and float(act[1, 2].sum()) == 0
    assert float(act[2, 3].sum()) == 1 and act[2, 3, 131 + 3] == 1 and float(act[2, 4].sum()) == 1 and act[2, 4, 5] == 1


# ---- end to end -----------------------------------------------------------------------------------------------------
def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _check_sampled(mtp, s_tensor, tokens, c_logits, seed):
    assert tokens.dtype == torch.int32 and tokens.shape == (c_logits.shape[0], 15, 2)
    act = mtp[s_tensor]
    assert torch.equal(act[..., :131].argmax(-1).int(), tokens[..., 0]) and torch.equal(act[..., 131:].argmax(-1).int(), tokens[..., 1])
    assert float(act.sum()) == 2.0 * 15 * act.shape[0]
    sil = mtp[~s_tensor]
    assert torch.equal(sil.argmax(-1)[:, 0], torch.full((sil.shape[0],), 129, device=DEV))
    assert torch.equal(sil.argmax(-1)[:, 1:], torch.full((sil.shape[0], 14), 130, device=DEV))
    assert float(sil.sum()) == 15.0 * sil.shape[0]
    assert torch.equal(tokens, ops.sample_tokens(c_logits, seed=seed))


@pytest.mark.parametrize("case", ["lmd2_tiny", "nb3_tiny"])
def test_generate_music_sampled_end_to_end(case):
    z, cfg = load_case(case)
    gg = np.load(os.path.join(GOLDEN, f"{case}_generate.npz"), allow_pickle=False)
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.eval()
    zs = torch.from_numpy(gg["gen/z"]).to(DEV)
    with torch.no_grad():
        _, c_logits = vae.decoder(zs, None)
        c_logits = c_logits.detach().contiguous().float()
        # without sampling arguments: the call as it was (the reference's capture of it holds no hash of the pianoroll, whose
        # logits differ from the reference's in their last bits; the bytes are those of the unchanged kernels on the
        # unchanged decoder output, and of the oracle's layout of them)
        mtp0, s0 = generate_music(vae, zs)
        assert torch.equal(s0.cpu(), torch.from_numpy(gg["gen/s_binary"]).bool())
        assert _sha(mtp0) == _sha(ops.mtp_from_logits(c_logits, s0)) == _sha(vae_cpu.mtp_from_logits(c_logits.cpu(), s0.cpu()))
        out = generate_music(vae, zs, seed=5)                                    # a seed alone samples nothing
        assert len(out) == 2 and _sha(out[0]) == _sha(mtp0)
        mtp_g, _, tok_g = generate_music(vae, zs, return_tokens=True)
        assert _sha(mtp_g) == _sha(mtp0) and torch.equal(tok_g, ops.sample_tokens(c_logits, temperature=0))
        # sampled
        mtp, s_tensor, tokens = generate_music(vae, zs, temperature=1, seed=7, return_tokens=True)
        assert torch.equal(s_tensor, s0) and mtp.shape == mtp0.shape
        _check_sampled(mtp, s_tensor, tokens, c_logits, 7)
        assert not torch.equal(tokens, tok_g)
        mtp_k, _ = generate_music(vae, zs, top_k=1)                              # temperature defaults to 1; top_k = 1 is greedy
        assert torch.equal(mtp_k, ops.mtp_from_tokens(tok_g, s0))
        # seed=None: torch's CPU generator, repeatable with torch.manual_seed
        torch.manual_seed(1234)
        a = generate_music(vae, zs, temperature=1.0, top_p=0.95, return_tokens=True)[2]
        b = generate_music(vae, zs, temperature=1.0, top_p=0.95, return_tokens=True)[2]
        torch.manual_seed(1234)
        c = generate_music(vae, zs, temperature=1.0, top_p=0.95, return_tokens=True)[2]
        assert torch.equal(a, c) and not torch.equal(a, b)


def test_generate_music_sampled_with_structure_conditioning():
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
        mtp0, s_out0 = generate_music(vae, zz, graph, s_tensor)
        assert s_out0 is s_tensor and torch.equal(mtp0[s_tensor], c_logits)
        mtp, s_out, tokens = generate_music(vae, zz, graph, s_tensor, temperature=1, seed=7, return_tokens=True)
    assert s_out is s_tensor
    _check_sampled(mtp, s_tensor, tokens, c_logits, 7)
