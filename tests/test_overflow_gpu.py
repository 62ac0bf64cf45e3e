"""The guarded optimizer step (include/polyphemus_hip.h, "guarded optimizer step"): `HipTrainer(..., overflow="skip")` skips
the Adam update on the device when the gradient it would consume holds an inf or a NaN, or when a split of the fp16 pair
format saturated during the step — what `scaler.step(optimizer)` of the reference's GradScaler does on found_inf
(training.py:123,152-162) — and `vae.poison_on_saturation` hands the same decision to the reference's own GradScaler."""
import math
import warnings

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.model import VAE
from polyphemus_amd.synthetic import synthetic_batch
from polyphemus_amd.trainer import HipTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, BETAS, EPS = 1e-3, (0.9, 0.98), 1e-9
# d = 128 with BatchNorm: the GCL products of both stacks run in the fp16 pair format (step_info()["h2"] == 3)
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)
# one element of a GCL weight: the weight planes are split at 2^4 (kH2WScale), 5000 * 16 > 65504 saturates, the forward stays finite
SAT_W = "encoder.c_encoder.graph_encoder.layers.0.weight"


def _pending(status) -> int:
    return int(status[ops.OVF_PENDING])


@pytest.mark.parametrize("n", [1, 3, 4096, 4097, 10_800_000])
@pytest.mark.parametrize("offset", [0, 1])
def test_nonfinite_check_flags_inf_and_nan_only(n, offset):
    """Random gradients, aligned and offset by one element (the scalar kernel): NaN, +inf and -inf at the first, a middle and
    the last position set the flag; finite extremes (+-FLT_MAX, denormals, -0.0) do not."""
    g = torch.Generator(device=DEV).manual_seed(n + offset)
    buf = torch.randn(n + offset, device=DEV, generator=g)
    x = buf[offset:]
    status = ops.overflow_status(DEV)
    ops.grad_nonfinite_check(x, status)
    assert _pending(status) == 0
    fmax = float(np.finfo(np.float32).max)
    for v in (fmax, -fmax, 1e-45, -1e-45, 1e-40, -0.0):
        for pos in sorted({0, n // 2, n - 1}):
            keep = x[pos].clone()
            x[pos] = v
            ops.grad_nonfinite_check(x, status)
            x[pos] = keep
    assert _pending(status) == 0, "a finite value was flagged"
    for v in (float("nan"), float("inf"), float("-inf")):
        for pos in sorted({0, n // 2, n - 1}):
            status.zero_()
            keep = x[pos].clone()
            x[pos] = v
            ops.grad_nonfinite_check(x, status)
            x[pos] = keep
            assert _pending(status) == ops.OVF_NONFINITE_BIT, (v, pos)


def _adam_buffers(n, offset, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mk = lambda: torch.randn(n + offset, device=DEV, generator=g)[offset:]
    p, m = mk(), mk() * 1e-3
    v = mk().abs() * 1e-6
    return p, m, v, g


@pytest.mark.parametrize("n,offset", [(8192, 0), (4099, 0), (4096, 1), (10_800_000, 0), (1, 0), (3, 1), (4, 0)])
def test_guarded_adam_applied_equals_adam_step_bitwise(n, offset):
    """No cause set: over several steps the parameters and both moments equal `ops.adam_step` at the same t bit for bit
    (float4 kernel and scalar kernel), the device t the check's last workgroup advances is the step number, nothing is
    counted as skipped, and the ticket is back at 0 after every decision."""
    p, m, v, g = _adam_buffers(n, offset, 5)
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    status = ops.overflow_status(DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in range(1, 6):
        grad = torch.randn(n + offset, device=DEV, generator=g)[offset:]
        ops.grad_nonfinite_check(grad, status, cnt[0:1], cnt[1:2], LR, *BETAS)
        ops.adam_step_guarded(p, grad, m, v, *BETAS, EPS, status, grad_scale=0.5)
        ops.adam_step(rp, grad, rm, rv, LR, *BETAS, EPS, t, grad_scale=0.5)
        assert cnt.tolist() == [t, 0] and int(status[ops.OVF_LAST]) == 0 and int(status[ops.OVF_TICKET]) == 0
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), t


def _host_scalars(t, lr, b1, b2):
    """pm_adam_step's host formula (optim.hip): float arguments widened to double, libm pow, rounded to float"""
    f = lambda x: float(np.float32(x))
    bc1 = 1.0 - math.pow(f(b1), float(t))
    bc2 = 1.0 - math.pow(f(b2), float(t))
    return np.float32(f(lr) / bc1), np.float32(1.0 / math.sqrt(bc2))


@pytest.mark.parametrize("lr,b1,b2", [(5e-6, 0.9, 0.98), (1e-3, 0.9, 0.999)])
def test_device_bias_scalars_equal_host_formula(lr, b1, b2):
    """The bias-correction scalars the guarded step computes on the device (double pow of ocml) equal those pm_adam_step
    computes on the host (libm), bit for bit, for every t in 1..100 000."""
    T = 100_000
    steps = torch.arange(1, T + 1, dtype=torch.int64, device=DEV)
    dev = ops.adam_bias_scalars(steps, lr, b1, b2).cpu().numpy()
    host = np.array([_host_scalars(t, lr, b1, b2) for t in range(1, T + 1)], dtype=np.float32)
    bad = np.nonzero((dev.view(np.uint32) != host.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {T} steps differ, first t = {bad[:8] + 1}: {dev[bad[:4]]} != {host[bad[:4]]}"


@pytest.mark.parametrize("cause", [ops.OVF_NONFINITE_BIT, ops.OVF_SATURATED_BIT])
def test_guarded_adam_skipped_stores_nothing(cause):
    """A cause set: the decision moves it to status[OVF_LAST]; parameters, exp_avg and exp_avg_sq are bitwise unchanged, t
    does not advance, the skip counter and the cause's counter advance by one."""
    for n, offset in ((8192, 0), (4097, 1)):
        p, m, v, g = _adam_buffers(n, offset, 9)
        status = ops.overflow_status(DEV)
        cnt = torch.tensor([7, 2], dtype=torch.int64, device=DEV)
        grad = torch.randn(n + offset, device=DEV, generator=g)[offset:]
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        status[ops.OVF_PENDING] = cause                 # (what the poison / an earlier check of the step recorded)
        ops.grad_nonfinite_check(grad, status, cnt[0:1], cnt[1:2], LR, *BETAS)
        ops.adam_step_guarded(p, grad, m, v, *BETAS, EPS, status)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert cnt.tolist() == [7, 3]
        st = status.tolist()
        assert st[ops.OVF_LAST] == cause and st[ops.OVF_PENDING] == 0
        assert (st[ops.OVF_N_SATURATED], st[ops.OVF_N_NONFINITE]) == ((1, 0) if cause == ops.OVF_SATURATED_BIT else (0, 1))
        # the next, clean step is applied at t = 8
        rp, rm, rv = p.clone(), m.clone(), v.clone()
        ops.grad_nonfinite_check(grad, status, cnt[0:1], cnt[1:2], LR, *BETAS)
        ops.adam_step_guarded(p, grad, m, v, *BETAS, EPS, status)
        ops.adam_step(rp, grad, rm, rv, LR, *BETAS, EPS, 8)
        assert cnt.tolist() == [8, 3] and torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv)


# ---------------------------------------------------------------------------------------------- trainer
def _model(seed=0):
    torch.manual_seed(seed)
    vae = VAE(**CFG, device=DEV).to(DEV)
    vae.train()
    vae.msg_dropout = 0.0
    return vae


def _batch(seed):
    b = synthetic_batch(24, 2, p=0.25, seed=seed).to(DEV)
    eps = torch.randn(24, CFG["d"], generator=torch.Generator().manual_seed(seed)).to(DEV)
    return b, eps


def _state(tr):
    return tr.vae.flat_params.detach().clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()


def _saturate(vae, value=5000.0):
    P = dict(vae.named_parameters())
    with torch.no_grad():
        old = float(P[SAT_W].view(-1)[3])
        P[SAT_W].view(-1)[3] = value
    return old


@pytest.mark.parametrize("native", [True, False])
def test_trainer_skip_policy_applies_finite_steps_exactly(native):
    """Finite batches with overflow="skip" (deterministic mode): after each step the parameters equal `ops.adam_step` of
    the step's pre-update state with the step's own gradient at the same t; no step is skipped; t is the step number."""
    with _lib.deterministic(True):
        vae = _model()
        tr = HipTrainer(vae, lr=LR, native=native, overflow="skip")
        for k in range(1, 4):
            p0, m0, v0 = _state(tr)
            tr.train_step(*_batch(50 + k))
            ops.adam_step(p0, tr.grads, m0, v0, LR, *BETAS, EPS, k)
            assert torch.equal(vae.flat_params, p0) and torch.equal(tr.exp_avg, m0) and torch.equal(tr.exp_avg_sq, v0), k
            assert int(tr.skipped_steps) == 0 and not bool(tr.last_update_skipped)
        assert tr.step_count == 3
        assert tr.overflow_stats() == {"skipped": 0, "non_finite": 0, "saturated": 0}


def test_trainer_skips_a_saturated_step_and_resumes(tmp_path):
    """A GCL weight of 5000 saturates the pair-format split of the weight planes (5000 * 2^4 > 65504) in the step's prologue,
    with a finite forward.  overflow="skip": the update is skipped (parameters, moments and t bitwise unchanged), the next
    step warns; overflow="ignore" applies it (today's behaviour).  With the weight restored the run trains on, t resuming
    where it stopped, and a checkpoint written after the skip carries the device t into a fresh trainer."""
    batch, eps = _batch(31)
    vae = _model()
    tr = HipTrainer(vae, lr=LR, overflow="skip")
    tr.train_step(*_batch(30))                                        # t = 1
    assert tr.step_info()["h2"] == 3                                  # the GCL products run in the pair format
    old = _saturate(vae)
    p0, m0, v0 = _state(tr)
    c0 = _lib.h2_clamp_events()
    out = tr.train_step(batch, eps)
    c1 = _lib.h2_clamp_events()
    assert c1 > c0, "the weight did not saturate the split"
    assert all(math.isfinite(v) for v in out.tolist()), "the forward was expected to stay finite"
    assert torch.equal(vae.flat_params, p0) and torch.equal(tr.exp_avg, m0) and torch.equal(tr.exp_avg_sq, v0)
    assert tr.step_count == 1 and int(tr.skipped_steps) == 1 and bool(tr.last_update_skipped)
    assert tr.overflow_stats() == {"skipped": 1, "non_finite": 0, "saturated": 1}
    ck = tmp_path / "skip.pt"
    tr.save_checkpoint(str(ck))

    # "ignore": the same step from the same state is applied (clipped gradient, no guard)
    vae_i = _model()
    tr_i = HipTrainer(vae_i, lr=LR)
    with torch.no_grad():
        vae_i.flat_params.copy_(p0)
    tr_i.exp_avg.copy_(m0); tr_i.exp_avg_sq.copy_(v0); tr_i.step_count = 1
    vae_i._step = vae._step
    tr_i.train_step(batch, eps)
    assert not torch.equal(vae_i.flat_params, p0) and tr_i.step_count == 2

    # restored weight: trains on at t = 2, and the skip of the step before is reported without a sync of its own
    P = dict(vae.named_parameters())
    with torch.no_grad():
        P[SAT_W].view(-1)[3] = old
    p1, m1, v1 = _state(tr)
    with pytest.warns(RuntimeWarning, match="skipped"):
        tr.train_step(*_batch(32))
    ops.adam_step(p1, tr.grads, m1, v1, LR, *BETAS, EPS, 2)
    assert torch.equal(vae.flat_params, p1) and tr.step_count == 2 and int(tr.skipped_steps) == 1
    assert not bool(tr.last_update_skipped)

    # checkpoint written after the skip: t = 1, not the 2 update attempts
    vae_r = _model(seed=5)
    tr_r = HipTrainer(vae_r, lr=LR, overflow="skip")
    tr_r.load_checkpoint(str(ck))
    assert tr_r.step_count == 1
    with torch.no_grad():
        dict(vae_r.named_parameters())[SAT_W].view(-1)[3] = old        # (the checkpoint holds the saturating weight)
    sd = torch.load(str(ck), weights_only=False)["optimizer_state_dict"]
    assert all(float(s["step"]) == 1.0 for s in sd["state"].values())
    p2, m2, v2 = _state(tr_r)
    tr_r.train_step(*_batch(33))
    ops.adam_step(p2, tr_r.grads, m2, v2, LR, *BETAS, EPS, 2)
    assert torch.equal(vae_r.flat_params, p2) and tr_r.step_count == 2


def test_trainer_skips_a_nonfinite_accumulated_gradient():
    """iters_to_accumulate = 2: a NaN in the accumulated gradient between the two micro-batches (GradScaler judges the
    accumulated .grad) skips the update."""
    vae = _model()
    tr = HipTrainer(vae, lr=LR, iters_to_accumulate=2, overflow="skip")
    p0, m0, v0 = _state(tr)
    tr.train_step(*_batch(40))
    tr.grad_accum[12345] = float("nan")
    tr.train_step(*_batch(41))
    assert torch.equal(vae.flat_params, p0) and torch.equal(tr.exp_avg, m0) and torch.equal(tr.exp_avg_sq, v0)
    assert tr.step_count == 0 and int(tr.skipped_steps) == 1
    assert tr.overflow_stats()["skipped"] == 1
    p1 = vae.flat_params.detach().clone()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tr.train_step(*_batch(42))
        tr.train_step(*_batch(43))
    assert tr.step_count == 1 and int(tr.skipped_steps) == 1 and not torch.equal(vae.flat_params, p1)


def test_trainer_skips_a_nonfinite_loss():
    """A non-finite loss through the public surface (trainer.beta = inf: the KLD term's gradient is inf / NaN): the update
    is skipped.  (No float of the step becomes an address, an index or a loop bound — the one float-to-integer conversion,
    the exponent in pm_pow2_scale, maps a non-finite bound to a scale of 1)"""
    vae = _model()
    tr = HipTrainer(vae, lr=LR, overflow="skip")
    tr.beta = float("inf")
    p0, m0, v0 = _state(tr)
    tr.train_step(*_batch(44))
    torch.cuda.synchronize()
    assert torch.equal(vae.flat_params, p0) and torch.equal(tr.exp_avg, m0) and torch.equal(tr.exp_avg_sq, v0)
    assert tr.step_count == 0 and int(tr.skipped_steps) == 1


def test_dropin_module_poisons_saturated_gradient_for_gradscaler():
    """The reference's loop, unchanged: `model(graph)`, the reference loss, `GradScaler.scale(loss).backward()`,
    `scaler.step(torch.optim.Adam)`.  With the saturating weight and `vae.poison_on_saturation = True` the returned gradient
    carries an inf, so GradScaler skips the step (parameters unchanged) and halves its scale."""
    from oracle import vae_cpu
    vae = _model()
    vae.poison_on_saturation = True
    _saturate(vae)
    batch, eps = _batch(31)
    opt = torch.optim.Adam(vae.parameters(), lr=LR, betas=BETAS, eps=EPS)
    scaler = torch.cuda.amp.GradScaler()
    s0 = scaler.get_scale()
    p0 = vae.flat_params.detach().clone()
    c0 = _lib.h2_clamp_events()
    (s_logits, c_logits), mu, lv = vae(batch)
    tot, _ = vae_cpu.losses(batch.s_tensor, s_logits, batch.c_tensor, c_logits, mu, lv)
    scaler.scale(tot).backward()
    assert _lib.h2_clamp_events() > c0
    scaler.step(opt)
    scaler.update()
    assert torch.equal(vae.flat_params, p0)
    assert scaler.get_scale() == s0 / 2
