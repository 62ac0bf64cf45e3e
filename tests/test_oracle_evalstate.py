"""Pin the CPU restatement (oracle/vae_cpu.py) in EVAL mode to the reference under a trained-like BatchNorm state
(tests/golden/<case>_evalstate.npz, oracle/make_golden.py evalstate): outputs, the eval-mode losses and accuracies, the
generation helpers.  Every other eval capture runs its norms at the initial state (running_mean 0, running_var 1, weight 1,
bias 0), where a norm that read the wrong statistics, or none, would go unnoticed; the last test guards the fixture against
degrading to that state."""
import json

import numpy as np
import pytest
import torch

from oracle import vae_cpu
from util import (assert_eval_c_logits_match, batch_from_golden, bn_keys, host_graph_from_binary, load_evalstate,
                  oracle_structure_logits, rel_err)
from polyphemus_amd import constants as C

CASES = ["lmd2_tiny", "nb3_tiny", "bnoff_tiny", "d128_l2"]


@pytest.fixture(autouse=True)
def _single_thread():
    """The fixtures were captured with one CPU thread (bit-reproducible reductions)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _params(z, sd):
    P, _ = vae_cpu.split_state({k: v.clone() for k, v in sd.items()}, [str(n) for n in z["param_names"]])
    return P


@pytest.mark.parametrize("case", CASES)
def test_eval_forward_under_trained_state(case):
    z, cfg, ze, sd = load_evalstate(case)
    g = batch_from_golden(z, cfg)
    P = _params(z, sd)
    with torch.no_grad():
        (s_logits, c_logits), mu, lv = vae_cpu.vae_forward(g, P, cfg, False, torch.from_numpy(z["in/eps"]))
        _, losses = vae_cpu.losses(g.s_tensor, s_logits, g.c_tensor, c_logits, mu, lv)
        accs = vae_cpu.accuracies(g.s_tensor, s_logits, g.c_tensor, c_logits, g.is_drum)
    for name, got in (("s_logits", s_logits), ("mu", mu), ("log_var", lv)):
        assert rel_err(got, ze[f"eval/{name}"]) < 1e-6, name
    assert_eval_c_logits_match(c_logits, ze, 1e-6, 1e-3)
    for k, v in json.loads(str(ze["metrics/losses"])).items():
        assert abs(float(losses[k]) - v) <= 1e-6 * max(1.0, abs(v)), (k, float(losses[k]), v)
    want = json.loads(str(ze["metrics/accs"]))
    assert set(accs) == set(want)
    for k, v in want.items():
        assert abs(accs[k] - v) < 1e-6, (k, accs[k], v)
    # the latent the conditioned generation capture decoded
    assert rel_err(torch.exp(0.5 * lv) * torch.from_numpy(z["in/eps"]) + mu, ze["cond/z"]) < 1e-6
    # eval mode leaves every buffer (and parameter) untouched
    for k, v in sd.items():
        assert torch.equal(P[k].detach(), v), k


@pytest.mark.parametrize("case", CASES)
def test_generation_under_trained_state(case):
    """generate.py:21-37 with s_cond = None through the oracle: the structure logits, the thresholded structure, the
    content decoder on the host-built graphs of that structure, and the pianoroll of those logits."""
    z, cfg, ze, sd = load_evalstate(case)
    P = _params(z, sd)
    zs = torch.from_numpy(ze["gen/z"])
    with torch.no_grad():
        s_logits = oracle_structure_logits(zs, P, cfg)
        s_bin = vae_cpu.binary_from_logits(s_logits)
        graph = host_graph_from_binary(s_bin, cfg["n_bars"])
        _, c_logits = vae_cpu.decoder_forward(zs, graph, P, cfg, False)
    assert rel_err(s_logits, ze["gen/s_logits"]) < 1e-6
    assert np.array_equal(s_bin.numpy().astype(np.uint8), ze["gen/s_binary"])
    assert c_logits.shape[0] == int(ze["gen/num_nodes"])
    assert rel_err(c_logits[:4], ze["gen/c_logits_head"]) < 1e-6
    scale = float(c_logits.abs().max()) * C.N_SLOTS * C.D_TOKEN_PAIR
    assert float(np.abs(c_logits.double().sum(dim=(-1, -2)).numpy() - ze["gen/c_logits_nodesum"]).max()) < 1e-6 * scale
    mtp = vae_cpu.mtp_from_logits(c_logits, s_bin)
    assert float(np.abs(mtp.double().sum(dim=(-1, -2)).numpy() - ze["gen/mtp_cellsum"]).max()) < 1e-6 * scale
    for k, v in sd.items():
        assert torch.equal(P[k].detach(), v), k


@pytest.mark.parametrize("case", CASES)
def test_evalstate_fixture_is_not_the_identity_state(case):
    """The fixture keeps its teeth: its norms hold statistics far from (0, 1), near-constant channels included, and its
    eval outputs are far from those of the initial state (tests/golden/<case>.npz eval/*)."""
    z, cfg, ze, sd = load_evalstate(case)
    keys = bn_keys(sd)
    assert len(keys) == sum(1 for k in ze.files if k.endswith(".running_mean"))
    assert min(float(sd[k + ".running_var"].min()) for k in keys) < 0.5
    assert max(float(sd[k + ".running_mean"].abs().max()) for k in keys) > 0.1
    for k in keys:                            # every norm moved: statistics, affine parameters, the batch counter
        assert not torch.equal(sd[k + ".running_mean"], torch.zeros_like(sd[k + ".running_mean"])), k
        assert not torch.equal(sd[k + ".running_var"], torch.ones_like(sd[k + ".running_var"])), k
        assert bool((sd[k + ".weight"] != 1).all()) and bool((sd[k + ".bias"] != 0).all()), k
        assert int(sd[k + ".num_batches_tracked"]) >= 3, k     # (bn_dur runs once per node group and forward)
    for name in ("s_logits", "mu", "log_var"):
        assert rel_err(ze[f"eval/{name}"], z[f"eval/{name}"]) > 0.1, name
    if "eval/c_logits_slots" in ze.files:
        want = ze["eval/c_logits_slots"]
        assert rel_err(want, z["eval/c_logits"][:, :want.shape[1]]) > 0.1
