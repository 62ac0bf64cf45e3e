"""Training accuracies of the step (HipTrainer(train_metrics=True)): the reference's `_accuracies` after every training batch
(training.py:174-179) from the logits the fused head trains on, counted on the device.

Kernel level: the metrics form of the fused un-embedding + cross-entropy against `pm_content_accuracy` on the logits the same
launch stores (integer for integer), and its loss / d_logits / bias gradients bit for bit against the default form.  Step
level: the counts of a full-size step against `content_accuracy` + `structure_metrics` on `step_outputs()`; the 9 accuracies
against the oracle on the reference's own training-mode logits; the history; the default path unchanged."""
import json
import math
import os

import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd._lib import call, lib, ptr, stream
from polyphemus_amd.model import VAE
from polyphemus_amd.synthetic import synthetic_batch
from polyphemus_amd.trainer import HipTrainer
from util import batch_from_golden, load_case, state_dict_from_golden

DEV = "cuda"
PP, PD = 130, 98


def _pad_beyond(cpu, S):
    cpu.tokens[:, S + 1:, 0] = PP                                 # slots past S are PAD in every node (what the step assumes)
    cpu.tokens[:, S + 1:, 1] = PD


def _scatter15(c_logits):
    N, S = c_logits.shape[:2]
    full = torch.zeros(N, 15, 230, device=c_logits.device)
    full[:, :S] = c_logits
    return full.contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("d,B,S,variant", [(32, 12, 5, "mixed"), (128, 20, 6, "mixed"), (256, 40, 6, "mixed"),
                                           (512, 12, 4, "mixed"), (256, 10, 5, "no_drums"), (256, 10, 5, "pad_slot")])
@pytest.mark.parametrize("rows", [False, True])
def test_fused_ce_metrics_match_content_accuracy(d, B, S, variant, rows):
    cpu = synthetic_batch(B, 2, p=0.3, seed=57 + d)
    _pad_beyond(cpu, S)
    if variant == "no_drums":
        cpu.is_drum = torch.zeros_like(cpu.is_drum)
    if variant == "pad_slot":                                     # one slot PAD in every node (both vocabularies)
        cpu.tokens[:, 2, 0] = PP
        cpu.tokens[:, 2, 1] = PD
    cpu.tokens[::7, 1, 0] = PP                                    # PAD in one vocabulary only
    b = cpu.to(DEV)
    plan = ops.plan_build(b.edge_index, b.edge_type, b.edge_dist, b.bars, b.batch, b.is_drum, b.tokens, b.n_bars,
                          b.s_tensor.shape[0], n_slots=S)
    N, dh, R = cpu.num_nodes, d // 2, cpu.num_nodes * S
    drum = b.is_drum.view(torch.uint8) if b.is_drum.dtype == torch.bool else b.is_drum
    drum = drum.contiguous()
    lists = torch.full((6, R), -7, dtype=torch.int32, device=DEV)
    counts_rl = torch.full((int(lib().pm_unembed_row_counts_len(N, S)),), -1, dtype=torch.int32, device=DEV)
    if rows:
        call("pm_unembed_row_lists", ptr(plan.tokens), ptr(plan.buf), N, plan.E, plan.G, d, S, ptr(lists), None, ptr(counts_rl),
             None, stream())
    torch.manual_seed(d + B)
    H = torch.randn(N, S, d, device=DEV)
    W = [torch.randn(v, dh, device=DEV) * 0.2 for v in (131, 131, 99)]
    bias = [torch.randn(v, device=DEV) for v in (131, 131, 99)]
    if d == 256:                                                   # exact ties: the lowest index must win in every kernel
        W[2][5] = W[2][40]
        bias[2][5] = bias[2][40]
    wpl = torch.empty(int(lib().pm_unembed_scratch_bytes(d)), dtype=torch.uint8, device=DEV)
    head = (ptr(H), ptr(W[0]), ptr(bias[0]), ptr(W[1]), ptr(bias[1]), ptr(W[2]), ptr(bias[2]), ptr(plan.tokens), ptr(plan.buf),
            N, plan.E, plan.G, d, S, 1.0, None)
    prev = _lib.is_deterministic()
    _lib.set_deterministic(True)
    try:
        res = []
        for met in (False, True):
            db = [torch.zeros(v, device=DEV) for v in (131, 131, 99)]
            out = torch.zeros(4, dtype=torch.float64, device=DEV)
            dl = torch.zeros(N, S, 230, device=DEV)
            lg = torch.zeros(N, S, 230, device=DEV)
            cnt = torch.full((16,), -5, dtype=torch.int64, device=DEV)          # every word is written
            verdict = torch.full((2 * R,), 7, dtype=torch.uint8, device=DEV)     # stale bytes are never read
            tail = (ptr(lg), ptr(dl), ptr(db[0]), ptr(db[1]), ptr(db[2]), ptr(out), ptr(wpl))
            rl = (ptr(lists), ptr(counts_rl)) if rows else ()
            name = "pm_unembed_ce" + ("_rows" if rows else "") + ("_metrics" if met else "")
            if met:
                call(name, *head, *tail, *rl, ptr(drum), ptr(verdict), ptr(cnt), stream())
            else:
                call(name, *head, *tail, *rl, stream())
            res.append((out, dl, db, lg, cnt))
    finally:
        _lib.set_deterministic(prev)
    (o0, dl0, db0, lg0, _), (o1, dl1, db1, lg1, cnt) = res
    assert torch.equal(o0, o1) and torch.equal(dl0, dl1) and torch.equal(lg0, lg1)
    for j in range(3):
        assert torch.equal(db0[j], db1[j]), j
    want = ops.content_accuracy(_scatter15(lg1), b.tokens.to(torch.int32).contiguous(), drum)
    got = cnt.tolist()
    assert got[:8] == want.tolist(), (got, want.tolist())
    assert got[8:] == [0] * 8
    assert got[1] > 0 and got[5] > 0
    if variant == "no_drums":
        assert got[2] == got[3] == 0 and math.isnan(ops.accuracies_from_counts(got)["pitch_drums"])
    # the S-aware count on materialised logits gives the same
    assert ops.content_accuracy_slots(lg1.contiguous(), b.tokens.to(torch.int32).contiguous(), drum).tolist() == got


def _model(d, layers, n_bars, seed=0):
    torch.manual_seed(seed)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=layers, d=d, n_bars=n_bars, resolution=8, device=torch.device(DEV)).to(DEV)
    vae.train()
    return vae


def _check_step_counts(vae, batch, fix_structure=False):
    tr = HipTrainer(vae, lr=5e-6, structure_loss_on_logits=fix_structure, train_metrics=True)
    tr.keep_logits = True
    tr.train_step(batch)
    (s_logits, c_logits), _, _ = tr.step_outputs()
    got = tr.last_train_counts.tolist()
    S = c_logits.shape[1]
    tok = batch.tokens.to(torch.int32).contiguous()
    drum = batch.is_drum.view(torch.uint8) if batch.is_drum.dtype == torch.bool else batch.is_drum
    assert bool((tok[:, S + 1:, 0] == PP).all()) and bool((tok[:, S + 1:, 1] == PD).all())
    cc = ops.content_accuracy(_scatter15(c_logits), tok, drum.contiguous()).tolist()
    s_t = batch.s_tensor.float().contiguous().reshape(-1)
    sc = ops.structure_metrics(s_logits.reshape(-1).contiguous() if fix_structure else s_t, s_t).tolist()
    assert got == cc + sc + [s_t.numel(), 0, 0, 0], (got, cc, sc)
    assert got[1] > 0 and got[5] > 0
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("fix", [False, True])
def test_full_size_step_counts_configs1(fix):
    vae = _model(256, 8, 2)
    batch = synthetic_batch(256, 2, p=0.25, seed=1234).to(DEV)
    tr = _check_step_counts(vae, batch, fix)
    assert tr.step_info()["fused_ce"] == 1 and tr.step_info()["planes"] == 1


@pytest.mark.gpu
def test_full_size_step_counts_dense_d512():
    vae = _model(512, 8, 2)
    _check_step_counts(vae, synthetic_batch(64, 2, p=0.25, seed=1234, dense=True).to(DEV))


@pytest.mark.gpu
def test_full_size_step_counts_lmd16():
    vae = _model(256, 8, 16)
    _check_step_counts(vae, synthetic_batch(64, 16, p=0.25, seed=1234).to(DEV))


@pytest.mark.gpu
def test_full_size_step_counts_unfused_head(monkeypatch):
    vae = _model(256, 8, 2)
    batch = synthetic_batch(256, 2, p=0.25, seed=1234).to(DEV)
    monkeypatch.setenv("PM_FUSED_CE", "0")
    lib().pm_vae_step_reload_switches()
    try:
        tr = _check_step_counts(vae, batch)
        assert tr.step_info()["fused_ce"] == 0
    finally:
        monkeypatch.delenv("PM_FUSED_CE")
        lib().pm_vae_step_reload_switches()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["lmd2_tiny", "nb3_tiny", "d128_l2"])
def test_train_accuracies_match_reference_golden(case):
    """The 9 accuracies of one `train_step` against `_accuracies` of the oracle on the reference's own training-mode outputs
    (train1/*), under the conditions of the golden training-step tests (message dropout 0, the golden eps)."""
    from oracle import vae_cpu
    z, cfg = load_case(case)
    vae = VAE(**cfg, device=torch.device(DEV)).to(DEV)
    vae.load_state_dict(state_dict_from_golden(z))
    vae.train()
    vae.msg_dropout = 0.0
    g = batch_from_golden(z, cfg).to(DEV)
    eps = torch.from_numpy(z["in/eps"]).to(DEV)
    optcfg = json.loads(str(z["opt"]))
    tr = HipTrainer(vae, lr_scheduler=optcfg["lr_scheduler"], train_metrics=True, **optcfg["optimizer"])
    tr.train_step(g, eps)
    (got,) = tr.read_train_accuracies()
    tok = g.tokens.long().cpu()
    c_tensor = torch.cat([torch.nn.functional.one_hot(tok[..., 0], 131), torch.nn.functional.one_hot(tok[..., 1], 99)], -1).float()
    c_logits = torch.from_numpy(z["train1/c_logits"]).float()
    s_t = g.s_tensor.float().cpu().reshape(torch.from_numpy(z["train1/s_logits"]).shape)
    want = vae_cpu.accuracies(s_t, torch.from_numpy(z["train1/s_logits"]).float(), c_tensor, c_logits, g.is_drum.cpu())
    for k, v in want.items():
        if math.isnan(v):
            assert math.isnan(got[k]), k
        else:
            assert abs(got[k] - v) <= 1e-6, (k, got[k], v)


@pytest.mark.gpu
def test_history_with_accumulation():
    vae = _model(128, 2, 2)
    batches = [synthetic_batch(16, 2, p=0.3, seed=300 + i).to(DEV) for i in range(5)]
    tr = HipTrainer(vae, lr=5e-6, iters_to_accumulate=2, train_metrics=True, metrics_capacity=5)
    tr.keep_logits = True
    want = []
    for b in batches:
        tr.train_step(b)
        (s_logits, c_logits), _, _ = tr.step_outputs()
        drum = b.is_drum.view(torch.uint8) if b.is_drum.dtype == torch.bool else b.is_drum
        s_t = b.s_tensor.float().contiguous().reshape(-1)
        cc = ops.content_accuracy_slots(c_logits.contiguous(), b.tokens.to(torch.int32).contiguous(), drum.contiguous())
        want.append(cc.tolist()[:8] + ops.structure_metrics(s_t, s_t).tolist() + [s_t.numel(), 0, 0, 0])
        assert tr.last_train_counts.tolist() == want[-1]
    with pytest.raises(RuntimeError, match="full"):
        tr.train_step(batches[0])
    got = tr.read_train_accuracies()
    assert len(got) == 5
    for g_, w in zip(got, want):
        wa = ops.accuracies_from_counts(w)
        assert all((math.isnan(g_[k]) and math.isnan(wa[k])) or g_[k] == wa[k] for k in wa)
    assert tr.read_train_accuracies() == []
    with pytest.raises(RuntimeError):
        tr.last_train_counts
    tr.train_step(batches[1])                                      # room again after the read
    assert len(tr.read_train_accuracies()) == 1


@pytest.mark.gpu
def test_default_unchanged_and_off_runs_no_metric_kernel():
    """Without the option no metric kernel runs (rocprofv3-free: the counts row of an armed state stays untouched by a
    disarmed trainer) and `last_train_counts` raises; in deterministic mode the parameters after 3 steps are bit-identical
    with the option on and off."""
    batch = synthetic_batch(32, 2, p=0.25, seed=77).to(DEV)
    prev = _lib.is_deterministic()
    _lib.set_deterministic(True)
    try:
        flats = []
        for on in (False, True):
            vae = _model(128, 2, 2, seed=3)
            tr = HipTrainer(vae, lr=1e-3, train_metrics=on)
            for _ in range(3):
                tr.train_step(batch)
            flats.append(vae.flat_params.detach().clone())
            if not on:
                with pytest.raises(RuntimeError):
                    tr.last_train_counts
                with pytest.raises(RuntimeError):
                    tr.read_train_accuracies()
            else:
                assert len(tr.read_train_accuracies()) == 3
        assert torch.equal(flats[0], flats[1])
    finally:
        _lib.set_deterministic(prev)
    # a state disarmed after an armed step: its next forward leaves the old row alone
    vae = _model(128, 2, 2)
    tr = HipTrainer(vae, lr=5e-6, train_metrics=True)
    tr.train_step(batch)
    row = tr.last_train_counts.clone()
    sentinel = torch.full((16,), -3, dtype=torch.int64, device=DEV)
    tr.last_train_counts.copy_(sentinel)
    call("pm_vae_step_set_metrics", tr.step.addr, None)
    tr.train_metrics = False
    tr.train_step(batch)
    torch.cuda.synchronize()
    assert torch.equal(tr._mhist[0], sentinel) and row[1] > 0


@pytest.mark.gpu
def test_python_orchestration_counts(monkeypatch):
    """native=False: the counts of `content_accuracy` / `structure_metrics` on the orchestration's own logits."""
    vae = _model(128, 2, 2)
    batch = synthetic_batch(16, 2, p=0.3, seed=5).to(DEV)
    tr = HipTrainer(vae, lr=5e-6, native=False, train_metrics=True)
    eng, cap = vae.engine, {}
    orig = eng.decoder_forward

    def spy(*a, **k):
        r = orig(*a, **k)
        cap["s"], cap["c"] = r[0].detach().clone(), r[1].detach().clone()
        return r
    monkeypatch.setattr(eng, "decoder_forward", spy)
    tr.train_step(batch)
    got = tr.last_train_counts.tolist()
    drum = batch.is_drum.view(torch.uint8) if batch.is_drum.dtype == torch.bool else batch.is_drum
    tok = batch.tokens.to(torch.int32).contiguous()
    c = cap["c"].contiguous()
    cc = (ops.content_accuracy(c, tok, drum.contiguous()) if c.shape[1] == 15 else
          ops.content_accuracy_slots(c, tok, drum.contiguous())[:8]).tolist()
    s_t = batch.s_tensor.float().contiguous().reshape(-1)
    assert got == cc + ops.structure_metrics(s_t, s_t).tolist() + [s_t.numel(), 0, 0, 0]
    assert got[1] > 0
    acc = tr.read_train_accuracies()
    assert len(acc) == 1 and list(acc[0]) == list(ops.ACCURACY_KEYS)
