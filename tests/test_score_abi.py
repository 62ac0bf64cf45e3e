"""Checks of the scores that need no GPU: pm_score_tokens and pm_score_structure are declared in include/polyphemus_hip.h
("Scores", behind "Note splicing"), exported by the library and bound in the ctypes table with the header's argument lists,
the ABI version is unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can
stand in for device addresses), the Python surface rejects bad arguments without a device, and the numpy restatement the GPU
tests compare with (tests/score_util.py) equals torch's CPU float64 cross_entropy / binary_cross_entropy_with_logits on the
inputs those tests use."""
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from polyphemus_amd import _lib
from score_util import (DUR_PAD, N_PITCH, PITCH_PAD, SLOTS, V_DUR_HIT, V_DUR_SET, V_PITCH_HIT, V_PITCH_SET, score_rows_ref,
                        score_structure_ref, score_tokens_ref, structure_case, structure_terms_ref, structures, targets_of,
                        token_case)
from test_abi import HEADER, header_prototypes

SIGS = {"pm_score_tokens": "ppipilpppppps", "pm_score_structure": "ppipps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
LOGITS, TOKENS, S, BAR_NODES, NODE_PTR, ROW_LOGP, VERDICT, LOGP, COUNTS, S_LOGITS = (0x10000000 + k * 0x100000 for k in range(10))
GOOD_T = dict(c_logits=LOGITS, tokens=TOKENS, tok_slots=15, s_tensor=S, G=3, N=40, bar_nodes=BAR_NODES, node_ptr=NODE_PTR,
              row_logp=ROW_LOGP, row_verdict=VERDICT, logp=LOGP, counts=COUNTS)
GOOD_S = dict(s_logits=S_LOGITS, s_tensor=S, G=3, logp=LOGP, counts=COUNTS)


def _tokens(**kw):
    return _lib.lib().pm_score_tokens(*{**GOOD_T, **kw}.values(), None)


def _structure(**kw):
    return _lib.lib().pm_score_structure(*{**GOOD_S, **kw}.values(), None)


def test_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig and len(getattr(L, name).argtypes) == len(sig) and name in _lib.EXPORTED
    src = open(HEADER).read()
    assert (src.index("------ Note splicing") < src.index("int pm_notes_splice") < src.index("------ Scores")
            < src.index("int pm_score_tokens") < src.index("int pm_score_structure") < src.index("------ message aggregation"))
    section = src[src.index("------ Scores"):src.index("------ message aggregation")]
    assert "training.py:298-347" in section and "training.py:438-468" in section
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())
BAD_T = ([{k: None} for k in GOOD_T if isinstance(GOOD_T[k], int) and GOOD_T[k] >= 0x10000000]
         + [dict(G=0), dict(G=-1), dict(N=-1), dict(N=-(1 << 40)), dict(tok_slots=14), dict(tok_slots=17), dict(tok_slots=0),
            dict(tok_slots=-15), dict(N=(1 << 31) // 15 + 1), dict(N=1 << 62), dict(G=1 << 24), dict(node_ptr=BAR_NODES),
            dict(tokens=TOKENS + 4), dict(row_logp=ROW_LOGP + 4), dict(logp=LOGP + 4), dict(c_logits=LOGITS + 2), dict(s_tensor=S + 1),
            dict(counts=COUNTS + 2), dict(bar_nodes=BAR_NODES + 1), dict(node_ptr=NODE_PTR + 3)])
BAD_S = ([{k: None} for k in ("s_logits", "s_tensor", "logp", "counts")]
         + [dict(G=0), dict(G=-5), dict(G=1 << 24), dict(logp=LOGP + 4), dict(s_logits=S_LOGITS + 2), dict(s_tensor=S + 1),
            dict(counts=COUNTS + 3)])


@pytest.mark.parametrize("bad", BAD_T, ids=_ids)
def test_score_tokens_rejects_on_the_host(bad):
    assert _tokens(**bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_S, ids=_ids)
def test_score_structure_rejects_on_the_host(bad):
    assert _structure(**bad) == PM_E_INVALID


def test_no_nodes_still_check_everything_else():
    """N == 0: the node-sized buffers may be NULL; the other arguments are checked as ever"""
    none = dict(N=0, c_logits=None, tokens=None, row_logp=None, row_verdict=None)
    for bad in (dict(logp=None), dict(counts=None), dict(s_tensor=None), dict(G=0), dict(tok_slots=3), dict(node_ptr=None),
                dict(bar_nodes=NODE_PTR)):
        assert _tokens(**none, **bad) == PM_E_INVALID


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import NoteBatch, score_graph, score_notes
    x, t15, t16 = torch.zeros(5, 15, 230), torch.zeros(5, 15, 2, dtype=torch.int32), torch.zeros(5, 16, 2, dtype=torch.int32)
    s = torch.zeros(1, 2, 4, 32)
    for bad in (x.double(), x[:, :14], x.view(5, 230, 15), x[0], x.numpy(), None):
        with pytest.raises(ValueError, match="c_logits"):
            ops.score_tokens(bad, t15, s)
    for bad in (t15.long(), t15[:, :14], t15[:, :, :1], torch.zeros(5, 17, 2, dtype=torch.int32), t15[0], t15.numpy(), t15.float()):
        with pytest.raises(ValueError, match="tokens"):
            ops.score_tokens(x, bad, s)
    with pytest.raises(ValueError, match="tokens has 4 nodes"):
        ops.score_tokens(x, t16[:4], s)
    for bad in (s[0], s.view(2, 1, 32, 4), torch.zeros(0, 2, 4, 32), torch.zeros(1, 0, 4, 32), s.numpy()):
        with pytest.raises(ValueError, match="s_tensor"):
            ops.score_tokens(x, t15, bad)
        with pytest.raises(ValueError, match="s_tensor"):
            ops.score_structure(s, bad)
    for bad in (s.double(), s[:, :1], s.view(2, 1, 4, 32), s.bool(), None):
        with pytest.raises(ValueError, match="s_logits"):
            ops.score_structure(bad, s)
    for tok in (t15, t16):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            ops.score_tokens(x, tok, s)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.score_structure(s, s.bool())

    # generate: before the model's encoder or the device is touched
    vae = types.SimpleNamespace(cfg=dict(n_bars=2, d=8), training=True)
    graph = types.SimpleNamespace(tokens=t16, s_tensor=torch.zeros(4, 4, 32), n_bars=2)          # B = 2
    for bad in (0, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError, match="samples"):
            score_graph(vae, graph, samples=bad)
    for bad in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="seed"):
            score_graph(vae, graph, seed=bad)
    for bad in (torch.zeros(8), torch.zeros(3, 8), torch.zeros(2, 7), torch.zeros(1, 3, 8), torch.zeros(0, 2, 8),
                torch.zeros(1, 1, 2, 8), torch.zeros(2, 8, dtype=torch.int64), np.zeros((2, 8), np.float32)):
        with pytest.raises(ValueError, match="z must be"):
            score_graph(vae, graph, z=bad)
    with pytest.raises(ValueError, match="n_bars"):
        score_graph(vae, types.SimpleNamespace(tokens=t16, s_tensor=torch.zeros(3, 4, 32), n_bars=3))
    with pytest.raises(ValueError, match="s_tensor"):
        score_graph(vae, types.SimpleNamespace(tokens=t16, s_tensor=torch.zeros(3, 4, 32), n_bars=2))
    with pytest.raises(ValueError, match="tokens"):
        score_graph(vae, types.SimpleNamespace(s_tensor=torch.zeros(4, 4, 32), n_bars=2))
    nb = NoteBatch.from_lists([[[(0, 60, 4)], [], [(5, 41, 2)], []]] * 2, 2, device="cpu")
    with pytest.raises(ValueError, match="NoteBatch"):
        score_notes(vae, graph)
    with pytest.raises(ValueError, match="n_bars"):
        score_notes(types.SimpleNamespace(cfg=dict(n_bars=3, d=8), training=True), nb)
    with pytest.raises(ValueError, match="samples"):
        score_notes(vae, nb, samples=0)
    with pytest.raises(ValueError, match="z must be"):
        score_notes(vae, nb, z=torch.zeros(3, 8))
    assert vae.training


TOKEN_CASES = [(name, slots) for name in structures() for slots in (15, 16)]


@pytest.mark.parametrize("name,slots", TOKEN_CASES)
def test_token_restatement_equals_torch_cross_entropy(name, slots):
    s = structures()[name]
    x, t = token_case(s, slots, seed=7)
    logp, counts, row_logp, verdict = score_tokens_ref(x, t, s)
    tgt = torch.from_numpy(targets_of(t).astype(np.int64))
    xt = torch.from_numpy(x).double()
    ce_p = F.cross_entropy(xt[..., :N_PITCH].reshape(-1, N_PITCH), tgt[..., 0].reshape(-1), ignore_index=PITCH_PAD, reduction="none")
    ce_d = F.cross_entropy(xt[..., N_PITCH:].reshape(-1, 99), tgt[..., 1].reshape(-1), ignore_index=DUR_PAD, reduction="none")
    want = -torch.stack([ce_p, ce_d], dim=-1).view(-1, SLOTS, 2).numpy()
    assert np.isfinite(want).all() and np.abs(row_logp - want).max() < 1e-12
    hit_p = (xt[..., :N_PITCH].argmax(-1) == tgt[..., 0]) & (tgt[..., 0] != PITCH_PAD)
    hit_d = (xt[..., N_PITCH:].argmax(-1) == tgt[..., 1]) & (tgt[..., 1] != DUR_PAD)
    want_v = (hit_p * V_PITCH_HIT + hit_d * V_DUR_HIT + (tgt[..., 0] != PITCH_PAD) * V_PITCH_SET + (tgt[..., 1] != DUR_PAD) * V_DUR_SET)
    assert np.array_equal(verdict, want_v.numpy().astype(np.uint8))
    # the planted rows are what they are meant to be
    v0 = verdict[0]
    assert v0[0] == 0 and v0[1] & (V_PITCH_SET | V_DUR_SET) == V_DUR_SET and v0[2] & (V_PITCH_SET | V_DUR_SET) == V_PITCH_SET
    assert v0[3] == 15 and v0[4] == V_PITCH_SET | V_DUR_SET                     # the first of the tied columns wins
    assert np.isneginf(x[0, 7]).sum() == 2 and x[0, 5, :N_PITCH].mean() > 70 and x[0, 6, N_PITCH:].mean() < -70
    # the sums: every node in exactly one (bar, track)
    G = s.reshape(-1, 128).shape[0]
    assert logp.shape == (G, 4, 2) and counts.shape == (G, 4, 6) and counts.dtype == np.int32
    assert np.array_equal(counts[..., 0], s.reshape(G, 4, 32).sum(-1)) and np.allclose(logp.sum((0, 1)), want.sum((0, 1)), rtol=0, atol=1e-9)
    assert counts[..., 1].sum() == int((tgt[..., 0] != PITCH_PAD).sum()) and counts[..., 5].sum() == int((hit_p & hit_d).sum())
    # nodes at N and beyond are ignored
    if x.shape[0] > 1:
        part = score_tokens_ref(x, t, s, N=x.shape[0] - 1)
        assert part[1][..., 0].sum() == x.shape[0] - 1


@pytest.mark.parametrize("G", [1, 3])
def test_structure_restatement_equals_torch_bce(G):
    x, y = structure_case(G, seed=11)
    logp, counts = score_structure_ref(x, y)
    want = F.binary_cross_entropy_with_logits(torch.from_numpy(x).double(), torch.from_numpy(y).double(), reduction="none")
    assert np.isfinite(want.numpy()).all()
    assert np.abs(structure_terms_ref(x, y) - want.numpy().reshape(-1, 4, 32)).max() < 1e-12
    assert np.abs(logp + want.view(G, 4, 32).sum(-1).numpy()).max() < 1e-10
    pred = torch.sigmoid(torch.from_numpy(x)).view(G, 4, 32).numpy() >= 0.5
    yy = y.reshape(G, 4, 32)
    assert np.array_equal(counts, np.stack([yy.sum(-1), pred.sum(-1), (yy & pred).sum(-1), (yy == pred).sum(-1)], -1))
    # the planted cells: a naive log(sigmoid) is -inf on the two that disagree with their target by 100, each in a track of
    # its own; the zeros are predicted on
    assert (np.abs(x) == 100).sum() == 4 and (x == 0).sum() == 3 and (logp[G - 1] < -100).sum() == 2
