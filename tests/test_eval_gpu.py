"""The eval-mode forward, `evaluate_batch` and generation (csrc kernels through polyphemus_amd/engine.py with
training=False) under TRAINED-LIKE BatchNorm state: running statistics of real batches, near-constant channels included,
and perturbed affine parameters.  Every other eval check runs its norms at the initial state, where eval BN is
x * 0.999995 and a norm that read the wrong layer's statistics, or none, passes.

(a) tests/golden/<case>_evalstate.npz (oracle/make_golden.py evalstate), captured from the reference: eval outputs, the
    eval-mode losses and accuracies, generation with and without structure conditioning.
(b) Full size (FULLSIZE configurations) against the fp64 / fp32 oracle in eval mode, on a state filled by 20 training-mode
    forwards and perturbed (util.trained_like_state; the oracle gets the same state dict): outputs with the criterion of the
    training outputs (tests/test_fullsize_gpu.py), `evaluate_batch`'s losses to 1e-6 and its accuracies up to the rows whose
    arg-max is a near tie in exact arithmetic.
(c) Generation at the reference's training configuration (training.json, d = 512), unconditioned and conditioned.
(d) The running statistics the native training step writes, at every FULLSIZE configuration, against the fp64 oracle's.

Tests (b) - (d) print one JSON line of their measured errors each."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import vae_cpu
from polyphemus_amd import constants as C
from polyphemus_amd.generate import generate_music, generate_z
from polyphemus_amd.model import VAE, _ReparamFn
from polyphemus_amd.synthetic import synthetic_batch
from polyphemus_amd.trainer import HipTrainer
from util import (FULLSIZE, REL_TOL, _as_dtype, assert_eval_c_logits_match, batch_from_golden, bn_keys, content_correct,
                  hip_fullsize_step, host_graph_from_binary, load_evalstate, oracle_eval_fullsize, oracle_fullsize,
                  oracle_structure_logits, rel_err, top2_margin, trained_like_state)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["lmd2_tiny", "nb3_tiny", "bnoff_tiny", "d128_l2"]
EVAL_FULLSIZE = ["configs1_lmd2_b256_d256", "training_json_b256_d512", "configs2_lmd16_b64_d256", "configs4_dense_shard_b8_d512"]
NEAR = 1e-5           # a logit margin below NEAR * max|logit| (fp64) is a tie at the fp32 arithmetic of either side


def _threads():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import host_cores
    torch.set_num_threads(host_cores())


def _model(cfg, sd):
    vae = VAE(**cfg, device=DEV).to(DEV)
    vae.load_state_dict(sd)
    vae.eval()
    return vae


def _eval_forward(vae, g, eps):
    """encoder / reparametrisation / decoder one by one (generate.py's surface)"""
    with torch.no_grad():
        mu, lv = vae.encoder(g)
        z = _ReparamFn.apply(mu, lv, eps)
        s_logits, c_logits = vae.decoder(z, g)
    return dict(s_logits=s_logits, c_logits=c_logits, mu=mu, log_var=lv)


def _assert_state_unchanged(vae, sd):
    for k, v in vae.state_dict().items():
        assert torch.equal(v.detach().cpu(), sd[k]), k


def _spy_decoder(vae):
    """record what `vae.decoder` returns on each call (generate_music discards its c_logits)"""
    seen = []
    fwd = vae.decoder.forward

    def spy(z, s=None):
        out = fwd(z, s)
        seen.append(out)
        return out
    vae.decoder.forward = spy
    return seen


def _cells_sum_scale(c_logits):
    return float(c_logits.abs().max()) * C.N_SLOTS * C.D_TOKEN_PAIR


# ---------------------------------------------------------------------------------------------------- (a) goldens
@pytest.mark.parametrize("case", CASES)
def test_eval_forward_and_metrics_match_reference_under_trained_state(case):
    z, cfg, ze, sd = load_evalstate(case)
    vae = _model(cfg, sd)
    g = batch_from_golden(z, cfg).to(DEV)
    eps = torch.from_numpy(z["in/eps"]).to(DEV)
    out = _eval_forward(vae, g, eps)
    for name in ("s_logits", "mu", "log_var"):
        assert out[name].shape == ze[f"eval/{name}"].shape
        assert rel_err(out[name], ze[f"eval/{name}"]) < REL_TOL, name
    assert_eval_c_logits_match(out["c_logits"], ze, REL_TOL, 2e-3)
    # evaluate_batch: the bounds of tests/test_model_gpu.py::test_evaluate_batch_matches_reference_metrics
    vae.train()
    losses, accs = HipTrainer(vae).evaluate_batch(g, eps)
    assert vae.training
    for k, v in json.loads(str(ze["metrics/losses"])).items():
        assert abs(losses[k] - v) <= REL_TOL * max(1.0, abs(v)), (k, losses[k], v)
    want = json.loads(str(ze["metrics/accs"]))
    assert set(accs) == set(want)
    for k, v in want.items():
        assert abs(accs[k] - v) < 1e-6, (k, accs[k], v)
    _assert_state_unchanged(vae, sd)


@pytest.mark.parametrize("case", CASES)
def test_generate_music_matches_reference_under_trained_state(case):
    """generate.py:21-37 unconditioned (structure-only pass, threshold, graph build, content decoder) and conditioned on the
    batch's own structure (the cond/* capture: the eval pass's latent decoded on that structure)."""
    z, cfg, ze, sd = load_evalstate(case)
    vae = _model(cfg, sd)
    zs = torch.from_numpy(ze["gen/z"]).to(DEV)
    with torch.no_grad():
        s_logits, c_logits = vae.decoder(zs, None)
        mtp, s_tensor = generate_music(vae, zs)
    assert rel_err(s_logits, ze["gen/s_logits"]) < REL_TOL
    want = torch.from_numpy(ze["gen/s_binary"]).bool()
    assert torch.equal(s_tensor.cpu(), want)
    assert float(np.abs(ze["gen/s_logits"]).min()) > 1e-5 * float(np.abs(ze["gen/s_logits"]).max())    # (no knife edges)
    assert c_logits.shape[0] == int(ze["gen/num_nodes"])
    assert rel_err(c_logits[:4], ze["gen/c_logits_head"]) < REL_TOL
    scale = _cells_sum_scale(c_logits)
    assert float(np.abs(c_logits.double().sum(dim=(-1, -2)).cpu().numpy() - ze["gen/c_logits_nodesum"]).max()) < REL_TOL * scale
    tok = torch.stack([c_logits[..., :C.N_PITCH_TOKENS].argmax(-1), c_logits[..., C.N_PITCH_TOKENS:].argmax(-1)], -1).cpu().numpy()
    assert (tok != ze["gen/c_argmax"]).mean() < 2e-3
    assert float(np.abs(mtp.double().sum(dim=(-1, -2)).cpu().numpy() - ze["gen/mtp_cellsum"]).max()) < REL_TOL * scale
    assert torch.equal(mtp.cpu(), vae_cpu.mtp_from_logits(c_logits.cpu(), s_tensor.cpu()))
    # conditioned
    B, nb = z["in/eps"].shape[0], cfg["n_bars"]
    s_cond = torch.from_numpy(z["in/s_tensor"]).view(B, nb, 4, 32).bool().to(DEV)
    seen = _spy_decoder(vae)
    with torch.no_grad():
        graph = vae.decoder._structure_from_binary(s_cond)
        mtp, s_out = generate_music(vae, torch.from_numpy(ze["cond/z"]).to(DEV), graph, s_cond)
    _, c_logits = seen[-1]
    assert s_out is s_cond
    assert float(np.abs(mtp.double().sum(dim=(-1, -2)).cpu().numpy() - ze["cond/mtp_cellsum"]).max()) < REL_TOL * _cells_sum_scale(c_logits)
    assert_eval_c_logits_match(c_logits, ze, REL_TOL, 2e-3)       # the same logits as the eval pass's
    assert torch.equal(mtp[s_cond], c_logits)
    _assert_state_unchanged(vae, sd)


# ---------------------------------------------------------------------------------------------------- (b) full size
_STATES = {}


def _state(name):
    if name not in _STATES:
        cfg, sd = trained_like_state(FULLSIZE[name], DEV)
        keys = bn_keys(sd)                       # non-trivial: the comparison below would not see a norm at identity
        for k in keys:
            assert int(sd[k + ".num_batches_tracked"]) >= 20, k
            assert float(sd[k + ".running_mean"].abs().max()) > 0 and bool((sd[k + ".running_var"] != 1).all()), k
        assert min(float(sd[k + ".running_var"].min()) for k in keys) < 0.5
        assert max(float(sd[k + ".running_mean"].abs().max()) for k in keys) > 0.1
        _STATES[name] = (cfg, sd)
    return _STATES[name]


def _counts(ok_p, ok_d, np_, nd_, drum):
    """the 5 content accuracies of `_accuracies` as (numerator, denominator) from per-row verdicts"""
    drum = drum.view(-1, 1).expand_as(np_)
    cp, cd = ok_p & np_, ok_d & nd_
    return {"note": ((cp & cd).sum(), np_.sum()), "pitch": (cp.sum(), np_.sum()),
            "pitch_drums": (cp[drum].sum(), np_[drum].sum()), "pitch_non_drums": (cp[~drum].sum(), np_[~drum].sum()),
            "dur": (cd.sum(), nd_.sum())}


@pytest.mark.parametrize("name", EVAL_FULLSIZE)
def test_eval_matches_oracle_at_full_size_under_trained_state(name):
    _threads()
    spec = FULLSIZE[name]
    cfg, sd = _state(name)
    cpu = synthetic_batch(spec["B"], spec["nb"], p=spec["p"], seed=spec["seed"], dense=spec["dense"])
    eps = torch.randn(spec["B"], spec["d"], generator=torch.Generator().manual_seed(99))
    vae = _model(cfg, sd)
    names = [n for n, _ in vae.named_parameters()]
    g = cpu.to(DEV)
    hip = {k: v.cpu() for k, v in _eval_forward(vae, g, eps.to(DEV)).items()}
    vae.train()
    losses, accs = HipTrainer(vae).evaluate_batch(g, eps.to(DEV))
    _assert_state_unchanged(vae, sd)
    del vae, g
    res, times = oracle_eval_fullsize(cfg, cpu, sd, names, eps)
    o64, l64, P64 = res["o64"]
    o32, _, P32 = res["o32"]
    for k, v in sd.items():                                     # (the oracle's eval mode leaves its state alone too)
        assert torch.equal(P64[k].to(v.dtype), v) and torch.equal(P32[k], v), k
    rep = {"name": name, "N": cpu.num_nodes, "outputs": {}, "losses": {}, "seconds": times}
    for k in ("s_logits", "c_logits", "mu", "log_var"):
        e = {"hip_vs_o64": rel_err(hip[k], o64[k]), "o32_vs_o64": rel_err(o32[k], o64[k]), "hip_vs_o32": rel_err(hip[k], o32[k])}
        rep["outputs"][k] = e
    for k, v in l64.items():
        rep["losses"][k] = abs(losses[k] - v) / max(1.0, abs(v))
    # accuracies: a row's verdict may differ from the fp64 oracle's only where its top-1 / top-2 margin is a near tie
    tokens = cpu.tokens
    c64 = o64["c_logits"]
    tie = top2_margin(c64) < NEAR * float(c64.abs().max())
    v64, vh = content_correct(c64, tokens), content_correct(hip["c_logits"], tokens)
    flips = ((v64[0] != vh[0]) | (v64[1] != vh[1])) & (v64[2] | v64[3])
    rep["near_tie_rows"], rep["rows"], rep["verdict_flips"] = int(tie.sum()), tie.numel(), int(flips.sum())
    drum = cpu.is_drum.bool()
    want = _counts(*v64, drum)
    n_tie = int((tie & (v64[2] | v64[3])).sum())
    acc_err = {}
    for k, (num, den) in want.items():
        acc_err[k] = abs(accs[k] * int(den) - int(num))
    ref_acc = vae_cpu.accuracies(cpu.s_tensor, o64["s_logits"], _as_dtype(cpu, torch.float64).c_tensor, c64, cpu.is_drum)
    rep["acc_count_err"] = acc_err
    print(json.dumps(rep))
    for k, e in rep["outputs"].items():
        assert e["hip_vs_o64"] < REL_TOL, (k, e)
        assert e["hip_vs_o32"] <= e["o32_vs_o64"] + REL_TOL, (k, e)
    for k, e in rep["losses"].items():
        assert e < 1e-6, (k, e, rep["losses"])
    assert not bool((flips & ~tie).any()), rep
    assert rep["near_tie_rows"] < 1e-3 * rep["rows"], rep
    for k, e in acc_err.items():
        assert e <= n_tie + 1e-6 * max(1, int(want[k][1])), (k, e, n_tie)
    for k in ("s_acc", "s_precision", "s_recall", "s_f1"):          # on the target itself (training.py:356); the oracle's
        assert abs(accs[k] - ref_acc[k]) < 1e-6, (k, accs[k], ref_acc[k])   # ratios are float32


# ---------------------------------------------------------------------------------------------------- (c) generation
def _structure_errors(s_hip, s64):
    near = s64.abs() < NEAR * float(s64.abs().max())
    want = vae_cpu.binary_from_logits(s64)
    diff = s_hip.cpu() != want
    return diff, near


def test_generation_matches_oracle_at_training_json_size_under_trained_state():
    """generate.py's model (training.json: B = 256, d = 512, 8 layers) on generate_z's latents: the structure logits and
    the thresholded structure against the fp64 oracle; the content logits against the oracle's eval decoder on the graphs
    the host builder makes of the HIP's own structure; the pianoroll laid out from exactly those logits.  Then again with
    a structure given (generate.py:205-237: one [n_bars, 4, 32] structure, an empty bar switched on, repeated over the
    batch)."""
    from oracle.vae_cpu import chunked_aggregation
    _threads()
    name = "training_json_b256_d512"
    spec = FULLSIZE[name]
    cfg, sd = _state(name)
    vae = _model(cfg, sd)
    names = [n for n, _ in vae.named_parameters()]
    torch.manual_seed(7)
    z = generate_z(spec["B"], spec["d"], DEV)
    z64 = z.cpu().double()
    P64, _ = vae_cpu.split_state({k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, names)
    rep = {"name": name}
    seen = _spy_decoder(vae)
    with torch.no_grad():
        mtp, s_tensor = generate_music(vae, z)
    s_hip, c_hip = seen[-1]
    with torch.no_grad():
        s64 = oracle_structure_logits(z64, P64, cfg)
    diff, near = _structure_errors(s_tensor, s64)
    rep["s_logits_vs_o64"] = rel_err(s_hip, s64)
    rep["structure_cells"], rep["near_zero_cells"], rep["structure_flips"] = diff.numel(), int(near.sum()), int(diff.sum())
    graph = host_graph_from_binary(s_tensor, cfg["n_bars"])
    assert graph.num_nodes == c_hip.shape[0] == int(s_tensor.sum())
    with torch.no_grad(), chunked_aggregation(65536, DEV):
        _, c64 = vae_cpu.decoder_forward(z64, _as_dtype(graph, torch.float64), P64, cfg, False)
    rep["N"], rep["c_logits_vs_o64"] = graph.num_nodes, rel_err(c_hip, c64)
    assert torch.equal(mtp[s_tensor], c_hip)                  # = vae_cpu.mtp_from_logits(c_hip, s_tensor), on the device
    sil = mtp[~s_tensor]
    assert float(sil.sum()) == 15.0 * sil.shape[0] and bool((sil[:, 0, 129] == 1).all()) and bool((sil[:, 1:, 130] == 1).all())
    del mtp, sil
    # conditioned
    s_one = torch.from_numpy(np.random.default_rng(5).random((cfg["n_bars"], 4, 32)) < 0.3)
    s_one[1] = False                                           # bar 1 empty -> [0,0] switched on
    s_cond = s_one.unsqueeze(0).repeat(spec["B"], 1, 1, 1).to(DEV)
    with torch.no_grad():
        g_cond = vae.decoder._structure_from_binary(s_cond)
        mtp, s_out = generate_music(vae, z, g_cond, s_cond)
    s_hip2, c_hip2 = seen[-1]
    assert s_out is s_cond and bool(s_cond[:, 1, 0, 0].all())
    graph = host_graph_from_binary(s_cond, cfg["n_bars"])
    with torch.no_grad(), chunked_aggregation(65536, DEV):
        s64c, c64c = vae_cpu.decoder_forward(z64, _as_dtype(graph, torch.float64), P64, cfg, False)
    rep["cond"] = {"N": graph.num_nodes, "s_logits_vs_o64": rel_err(s_hip2, s64c), "c_logits_vs_o64": rel_err(c_hip2, c64c)}
    assert torch.equal(mtp[s_cond], c_hip2)
    print(json.dumps(rep))
    _assert_state_unchanged(vae, sd)
    assert rep["s_logits_vs_o64"] < REL_TOL and rep["c_logits_vs_o64"] < REL_TOL, rep
    assert not bool((diff & ~near).any()), rep
    assert rep["near_zero_cells"] < 1e-3 * rep["structure_cells"], rep
    assert rep["cond"]["s_logits_vs_o64"] < REL_TOL and rep["cond"]["c_logits_vs_o64"] < REL_TOL, rep


# ---------------------------------------------------------------------------------------------------- (d) running stats
@pytest.mark.parametrize("name", list(FULLSIZE))
def test_native_step_running_statistics_match_oracle_at_full_size(name):
    """What eval consumes: the running_mean / running_var the native training step writes (momentum 0.1 from the initial
    state), per tensor against the fp64 oracle's step on the same batch, weights, eps and dropout mask."""
    _threads()
    spec = FULLSIZE[name]
    live = {}
    run = hip_fullsize_step(spec, keep=live)
    hip_sd = {k: v.detach().cpu().clone() for k, v in live["vae"].state_dict().items()}
    live.clear()
    states = {}
    oracle_fullsize(spec, run, dtypes=(("o64", torch.float64),), states=states)
    s64 = states["o64"]
    err = {}
    for k in bn_keys(hip_sd):
        assert int(hip_sd[k + ".num_batches_tracked"]) == int(s64[k + ".num_batches_tracked"]), k
        for t in ("running_mean", "running_var"):
            err[f"{k}.{t}"] = rel_err(hip_sd[f"{k}.{t}"], s64[f"{k}.{t}"])
    worst = max(err, key=err.get)
    print(json.dumps({"name": name, "tensors": len(err), "worst": worst, "worst_err": err[worst]}))
    for k, e in err.items():
        assert e < REL_TOL, (k, e)
