"""The exponential moving average of the parameters (include/polyphemus_hip.h, "exponential moving average of the
parameters"): `pm_adam_step_ema` leaves the parameters and both moments exactly as the three Adam entries leave them and
moves the average towards the parameter it stored; `pm_buffer_swap` exchanges two buffers in place; and
`HipTrainer(..., ema_decay=...)` with `ema_weights()`, `evaluate*(ema=True)`, `ema_state_dict()` and the checkpoint."""
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
# 4096 * 256 * 4 + 4: the smallest size that sends a float4 thread round the grid-stride loop a second time
SIZES = [1, 3, 4, 4096, 4097, 4_194_308]
# e + w (p - e) in fp32: three roundings (p - e, the product, the sum) of magnitudes <= max(|e|, |p|), <= 1.5 ulp <= 2^-22 max;
# an FMA contraction drops one of them
BOUND = 2.0 ** -22
MODES = ["plain", "guard", "clip", "guard+clip"]


def _f32(x) -> float:
    return float(np.float32(x))


# where the buffers start: all 16-byte aligned; the average alone one element into its allocation (it must not change which
# kernel p, m and v go through: the float4 one moves it as four floats); all five one element in (the scalar kernel)
OFFSETS = [0, 1, "all"]


def _at(x, k):
    """a copy of `x` that starts k elements into its own allocation"""
    out = torch.empty(x.numel() + k, device=DEV)[k:]
    assert out.data_ptr() % 16 == 4 * k
    return out.copy_(x)


def _buffers(n, offset, seed):
    """(p, m, v, average, generator, k): k = the element offset of p, m, v and of the gradients `_grad` makes for them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    k, ke = (1, 1) if offset == "all" else (0, offset)
    mk = lambda kk: _at(torch.randn(n, device=DEV, generator=g), kk)
    p, m = mk(k), mk(k).mul_(1e-3)
    v = mk(k).abs_().mul_(1e-6)
    return p, m, v, mk(ke), g, k


def _grad(n, g, k):
    return _at(torch.randn(n, device=DEV, generator=g), k)


class _Stepper:
    """One optimizer update in a mode, on the reference buffers through the entry the mode had before the average and on the
    test buffers through `adam_step_ema`, from one read of the gradient (one decision, one clip block)."""

    def __init__(self, mode):
        self.guard, self.clip = "guard" in mode, "clip" in mode
        self.status = ops.overflow_status(DEV)
        self.cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.block = ops.clip_block(DEV)

    def __call__(self, t, grad, ref, got, ema, w, gs=0.5):
        status = self.status if self.guard else None
        if self.guard and self.clip:
            ops.grad_nonfinite_check_sumsq(grad, self.status, self.block, self.cnt[0:1], self.cnt[1:2], LR, *BETAS)
        elif self.guard:
            ops.grad_nonfinite_check(grad, self.status, self.cnt[0:1], self.cnt[1:2], LR, *BETAS)
        elif self.clip:
            ops.grad_sumsq(grad, self.block)
        if self.clip:                                                    # half the norm of what Adam consumes: coef < 1
            ops.grad_clip_finish(self.block, _f32(0.5 * gs * float(grad.double().norm())), gs)
            assert 0.49 < float(self.block[ops.CLIP_COEF]) < 0.51
            ops.adam_step_clipped(*ref[:1], grad, *ref[1:], LR, *BETAS, EPS, t, self.block, status)
        elif self.guard:
            ops.adam_step_guarded(*ref[:1], grad, *ref[1:], *BETAS, EPS, self.status, grad_scale=gs)
        else:
            ops.adam_step(*ref[:1], grad, *ref[1:], LR, *BETAS, EPS, t, grad_scale=gs)
        ops.adam_step_ema(*got[:1], grad, *got[1:], ema, LR, *BETAS, EPS, t, w, grad_scale=gs,
                          clip=self.block if self.clip else None, status=status)


def _check_average(e_prev, p_new, e_new, w, what):
    """on the host in float64, from the kernel's own fp32 buffers read back"""
    e0, p1, e1 = (x.cpu().double() for x in (e_prev, p_new, e_new))
    want = e0 + w * (p1 - e0)
    excess = (e1 - want).abs() - BOUND * torch.maximum(e0.abs(), p1.abs())
    assert float(excess.max()) <= 0.0, (what, float(excess.max()))


# ---------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("mode", MODES)
def test_adam_step_ema_leaves_p_m_v_as_the_entry_without_the_average(n, offset, mode):
    """Three consecutive updates from the same inputs: `params`, `exp_avg` and `exp_avg_sq` are bitwise those of
    `adam_step` / `adam_step_guarded` / `adam_step_clipped` (coef < 1) — also where the average alone is not 16-byte aligned
    (the scalar and the float4 kernel differ in a last bit of exp_avg: the average's alignment must not choose between
    them) — and after every update the average (decay 0.999) is within the bound of the float64 recurrence."""
    w = ops.ema_weight(0.999)
    p, m, v, e, g, k = _buffers(n, offset, 5 + n % 97)
    ref = [_at(p, k), _at(m, k), _at(v, k)]
    step = _Stepper(mode)
    for t in range(1, 4):
        grad = _grad(n, g, k)
        e_prev = e.clone()
        step(t, grad, ref, [p, m, v], e, w)
        assert torch.equal(p, ref[0]) and torch.equal(m, ref[1]) and torch.equal(v, ref[2]), t
        assert not torch.equal(e, e_prev)
        _check_average(e_prev, p, e, w, t)
    if step.guard:
        assert step.cnt.tolist() == [3, 0]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", OFFSETS)
def test_average_follows_the_float64_recurrence_at_decay_one_half(n, offset):
    w = ops.ema_weight(0.5)
    assert w == 0.5
    p, m, v, e, g, k = _buffers(n, offset, 11 + n % 89)
    for t in range(1, 4):
        grad = _grad(n, g, k)
        e_prev = e.clone()
        ops.adam_step_ema(p, grad, m, v, e, LR, *BETAS, EPS, t, w)
        _check_average(e_prev, p, e, w, t)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", OFFSETS)
def test_a_weight_of_one_copies_the_parameters(n, offset):
    p, m, v, e, g, k = _buffers(n, offset, 3)
    ops.adam_step_ema(p, _grad(n, g, k), m, v, e, LR, *BETAS, EPS, 1, 1.0)
    assert torch.equal(e, p)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("clip", [False, True])
def test_a_skipped_step_stores_nothing_into_the_average_either(n, offset, clip):
    """A status block whose PM_OVF_LAST holds a cause: params, both moments AND the average are bitwise unchanged."""
    p, m, v, e, g, k = _buffers(n, offset, 9)
    grad = _grad(n, g, k)
    keep = [x.clone() for x in (p, m, v, e)]
    status = ops.overflow_status(DEV)
    status[ops.OVF_LAST] = ops.OVF_NONFINITE_BIT
    block = None
    if clip:
        block = ops.clip_block(DEV)
        ops.grad_sumsq(grad, block)
        ops.grad_clip_finish(block, 1.0)
    ops.adam_step_ema(p, grad, m, v, e, LR, *BETAS, EPS, 0, 0.5, clip=block, status=status)
    for a, b in zip((p, m, v, e), keep):
        assert torch.equal(a, b)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1])
def test_buffer_swap_exchanges_exactly_and_twice_restores(n, offset):
    """Both aligned (float4 at n % 4 == 0), and one of them one element into its allocation (scalar)."""
    g = torch.Generator(device=DEV).manual_seed(n + offset)
    a = torch.randn(n, device=DEV, generator=g)
    b = _at(torch.randn(n, device=DEV, generator=g), offset)
    a0, b0 = a.clone(), b.clone()
    ops.buffer_swap(a, b)
    assert torch.equal(a, b0) and torch.equal(b, a0)
    ops.buffer_swap(a, b)
    assert torch.equal(a, a0) and torch.equal(b, b0)


def test_ops_wrappers_check_their_arguments():
    p, m, v, e, g, k = _buffers(8, 0, 1)
    grad = _grad(8, g, k)
    with pytest.raises(ValueError, match="ema_weight"):
        ops.adam_step_ema(p, grad, m, v, e, LR, *BETAS, EPS, 1, 0.0)
    with pytest.raises(ValueError, match="as many elements"):
        ops.adam_step_ema(p, grad, m, v, e[:4], LR, *BETAS, EPS, 1, 0.5)
    with pytest.raises(TypeError):
        ops.adam_step_ema(p, grad, m, v, e.double(), LR, *BETAS, EPS, 1, 0.5)
    with pytest.raises(_lib.HipExtensionError, match="PM_E_INVALID"):
        ops.adam_step_ema(p, grad, m, v, p, LR, *BETAS, EPS, 1, 0.5)
    with pytest.raises(ValueError, match="same number"):
        ops.buffer_swap(p, e[:4])
    with pytest.raises(_lib.HipExtensionError, match="PM_E_INVALID"):
        ops.buffer_swap(p, p)


# ---------------------------------------------------------------------------------------------- trainer
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)     # tests/test_zz_gradclip_dp_gpu.py


def _model(seed=0):
    torch.manual_seed(seed)
    vae = VAE(**CFG, device=DEV).to(DEV)
    vae.train()
    vae.msg_dropout = 0.0
    return vae


def _batch(seed):
    b = synthetic_batch(12, 2, p=0.25, seed=seed).to(DEV)
    eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(seed)).to(DEV)
    return b, eps


def _flat(tr):
    return tr.vae.flat_params.detach().clone()


@pytest.mark.parametrize("bad", [True, -0.1, 1.0, 1.5, "0.9", 1 - 1e-12])
def test_trainer_rejects_bad_ema_decay(bad):
    with pytest.raises(ValueError, match="ema_decay"):
        HipTrainer(_model(), ema_decay=bad)


def test_trainer_without_the_option_has_no_average():
    tr = HipTrainer(_model(), lr=LR)
    assert tr.ema is None and tr.ema_decay is None
    batch, eps = _batch(1)
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.evaluate([batch], ema=True)
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.evaluate_batch(batch, eps, ema=True)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.ema_state_dict()


@pytest.mark.parametrize("native", [True, False])
def test_trainer_average_matches_torch_averaged_model(native):
    """`torch.optim.swa_utils.AveragedModel` with `get_ema_multi_avg_fn(0.9)` over CPU copies of the parameters: its first
    `update_parameters` copies (the initial weights: our starting point), then one call behind each of three `train_step`s
    with the trainer's read-back parameters.  `trainer.ema` agrees within the per-step bound accumulated over the three."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    vae = _model()
    tr = HipTrainer(vae, lr=LR, native=native, ema_decay=0.9)
    names = vae._param_names
    P = dict(vae.named_parameters())
    spans = [(vae._offsets[n], P[n].numel()) for n in names]

    holder = torch.nn.Module()
    holder.params = torch.nn.ParameterList([torch.nn.Parameter(torch.empty(k)) for _, k in spans])

    def read_back():
        flat = vae.flat_params.detach().cpu()
        with torch.no_grad():
            for q, (o, k) in zip(holder.params, spans):
                q.copy_(flat[o:o + k])
        return flat

    seen = read_back().abs()
    assert torch.equal(tr.ema, vae.flat_params)
    avg = AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    avg.update_parameters(holder)
    for k in range(3):
        tr.train_step(*_batch(20 + k))
        seen = torch.maximum(seen, read_back().abs())
        avg.update_parameters(holder)
        seen = torch.maximum(seen, tr.ema.cpu().abs())
    assert int(avg.n_averaged) == 4 and not torch.equal(tr.ema, vae.flat_params)
    got = tr.ema.cpu()
    for q, (o, k) in zip(avg.module.params, spans):
        excess = (got[o:o + k].double() - q.detach().double()).abs() - 3 * BOUND * seen[o:o + k].double()
        assert float(excess.max()) <= 0.0, float(excess.max())


def test_trainer_decay_zero_tracks_the_parameters_exactly():
    tr = HipTrainer(_model(), lr=LR, ema_decay=0)
    for k in range(3):
        p0 = _flat(tr)
        tr.train_step(*_batch(30 + k))
        assert torch.equal(tr.ema, tr.vae.flat_params) and not torch.equal(tr.ema, p0)


def test_trainer_accumulation_moves_the_average_once_per_update():
    tr = HipTrainer(_model(), lr=LR, iters_to_accumulate=2, ema_decay=0.9)
    for k in range(4):
        e0 = tr.ema.clone()
        tr.train_step(*_batch(40 + k))
        assert torch.equal(tr.ema, e0) == (k % 2 == 0), k
    assert tr.step_count == 2


def test_trainer_guard_skips_the_average_with_the_update():
    """overflow="skip": a non-finite gradient (trainer.beta = inf, as tests/test_overflow_gpu.py) leaves the average, the
    parameters and t bit-unchanged; the next clean step moves all of them."""
    tr = HipTrainer(_model(), lr=LR, overflow="skip", ema_decay=0.9)
    tr.train_step(*_batch(50))
    e0, p0 = tr.ema.clone(), _flat(tr)
    assert tr.step_count == 1 and not torch.equal(e0, p0)
    tr.beta = float("inf")
    tr.train_step(*_batch(51))
    assert torch.equal(tr.ema, e0) and torch.equal(tr.vae.flat_params, p0)
    assert tr.step_count == 1 and int(tr.skipped_steps) == 1
    tr.beta = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                  # (the skip of the step before is reported here)
        tr.train_step(*_batch(52))
    assert not torch.equal(tr.ema, e0) and not torch.equal(tr.vae.flat_params, p0)
    assert tr.step_count == 2 and int(tr.skipped_steps) == 1


def test_ema_weights_context_swaps_in_place_and_back(tmp_path):
    tr = HipTrainer(_model(), lr=LR, ema_decay=0.5)
    for k in range(2):
        tr.train_step(*_batch(60 + k))
    vae = tr.vae
    e0, p0, at = tr.ema.clone(), _flat(tr), vae.flat_params.data_ptr()
    assert not torch.equal(e0, p0)
    with tr.ema_weights() as model:
        assert model is vae
        assert torch.equal(vae.flat_params, e0) and torch.equal(tr.ema, p0) and vae.flat_params.data_ptr() == at
        w = "encoder.c_encoder.graph_encoder.layers.1.weight"                 # the parameter views see the average
        o = vae._offsets[w]
        q = dict(vae.named_parameters())[w].detach()
        assert torch.equal(q.reshape(-1), e0[o:o + q.numel()])
        with pytest.raises(RuntimeError, match="ema_weights"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step(*_batch(62))
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.save_checkpoint(str(tmp_path / "inside.pt"))
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.load_checkpoint(str(tmp_path / "inside.pt"))
        assert torch.equal(vae.flat_params, e0) and torch.equal(tr.ema, p0)   # (the refusals moved nothing)
    assert torch.equal(vae.flat_params, p0) and torch.equal(tr.ema, e0) and vae.flat_params.data_ptr() == at
    with pytest.raises(KeyError, match="inside"):
        with tr.ema_weights():
            assert torch.equal(vae.flat_params, e0)
            raise KeyError("inside")
    assert torch.equal(vae.flat_params, p0) and torch.equal(tr.ema, e0)
    tr.train_step(*_batch(62))                                               # and the trainer trains on
    assert tr.step_count == 3


def test_evaluation_on_the_average_is_that_of_a_model_loaded_from_ema_state_dict():
    """Deterministic mode (bit-reproducible kernels, so the repeat-call difference measured below is the arithmetic's own).
    decay 0.5 at lr 1e-2 over three steps: the average is far from the parameters; `evaluate_batch(..., ema=True)` gives the
    losses of a second model loaded from `ema_state_dict()` — same kernels on the same values — and the same accuracies,
    and not those of the live weights."""
    with _lib.deterministic(True):
        tr = HipTrainer(_model(), lr=1e-2, ema_decay=0.5)
        for k in range(3):
            tr.train_step(*_batch(70 + k))
        assert not torch.equal(tr.ema, tr.vae.flat_params)
        batch, eps = _batch(73)
        sd = tr.ema_state_dict()
        # the reference's key layout (255 keys at 8 layers), the aliases of the shared edge network included
        assert list(sd) == list(tr.vae.state_dict()) and any(".layers.1.nn." in k for k in sd)
        p0, e0 = _flat(tr), tr.ema.clone()
        got_l, got_a = tr.evaluate_batch(batch, eps, ema=True)
        assert torch.equal(tr.vae.flat_params, p0) and torch.equal(tr.ema, e0) and tr.vae.training
        live_l, _ = tr.evaluate_batch(batch, eps)

        second = _model(seed=9)
        second.load_state_dict(sd)
        tr2 = HipTrainer(second, lr=1e-2)
        want_l, want_a = tr2.evaluate_batch(batch, eps)
        again_l, _ = tr2.evaluate_batch(batch, eps)
        for k in want_l:
            allowed = max(abs(again_l[k] - want_l[k]), 1e-12 * abs(want_l[k]))
            print(f"{k}: ema {got_l[k]!r} second {want_l[k]!r} repeat {again_l[k]!r} live {live_l[k]!r}")
            assert abs(got_l[k] - want_l[k]) <= allowed, (k, got_l[k], want_l[k], allowed)
        assert got_a == want_a
        assert abs(got_l["tot"] - live_l["tot"]) > 1e-6 * abs(live_l["tot"])
        eval_l, eval_a = tr.evaluate([batch], ema=True)                       # the loader form draws its own eps
        assert set(eval_l) == set(got_l) and eval_a["s_acc"] == got_a["s_acc"]


def test_checkpoint_round_trip_carries_the_average(tmp_path):
    tr = HipTrainer(_model(), lr=LR, ema_decay=0.9)
    for k in range(3):
        tr.train_step(*_batch(80 + k))
    ck = str(tmp_path / "ema.pt")
    tr.save_checkpoint(ck, epoch=1)
    raw = torch.load(ck, weights_only=False)
    assert raw["ema"] == {"decay": 0.9, "n_averaged": 3}
    assert list(raw["ema_model_state_dict"]) == list(raw["model_state_dict"]) == list(tr.vae.state_dict())
    w = "decoder.c_decoder.graph_decoder.layers.1.weight"
    o = tr.vae._offsets[w]
    assert torch.equal(raw["ema_model_state_dict"][w].reshape(-1), tr.ema[o:o + raw["model_state_dict"][w].numel()].cpu())
    bn = next(k for k in raw["model_state_dict"] if k.endswith("running_var"))
    assert torch.equal(raw["ema_model_state_dict"][bn], raw["model_state_dict"][bn])       # buffers: the live model's

    # the same option: the average comes back bit for bit, and n_averaged goes on counting
    tr_r = HipTrainer(_model(seed=5), lr=LR, ema_decay=0.9)
    rest = tr_r.load_checkpoint(ck)
    assert torch.equal(tr_r.ema, tr.ema) and torch.equal(tr_r.vae.flat_params, tr.vae.flat_params)
    assert "ema" not in rest and "ema_model_state_dict" not in rest and rest["epoch"] == 1
    ck2 = str(tmp_path / "ema2.pt")
    tr_r.train_step(*_batch(83))
    tr_r.save_checkpoint(ck2)
    assert torch.load(ck2, weights_only=False)["ema"]["n_averaged"] == 4

    # no option: the entries stay in the remainder, and the written dict is that of a trainer built without the argument
    tr_off = HipTrainer(_model(seed=6), lr=LR, ema_decay=None)
    rest = tr_off.load_checkpoint(ck)
    assert rest["ema"] == {"decay": 0.9, "n_averaged": 3}
    assert list(rest["ema_model_state_dict"]) == list(raw["model_state_dict"])
    ck_off, ck_plain = str(tmp_path / "off.pt"), str(tmp_path / "plain.pt")
    tr_off.save_checkpoint(ck_off)
    HipTrainer(_model(seed=7), lr=LR).save_checkpoint(ck_plain)
    keys_off, keys_plain = (set(torch.load(f, weights_only=False)) for f in (ck_off, ck_plain))
    assert keys_off == keys_plain and "ema" not in keys_off and "ema_model_state_dict" not in keys_off

    # the option, a file without an average: it starts from the loaded parameters
    tr_new = HipTrainer(_model(seed=8), lr=LR, ema_decay=0.9)
    assert not torch.equal(tr_new.ema, tr_off.vae.flat_params)
    tr_new.load_checkpoint(ck_off)
    assert torch.equal(tr_new.ema, tr_new.vae.flat_params) and torch.equal(tr_new.ema, tr_off.vae.flat_params)
    tr_new.train_step(*_batch(84))
    tr_new.save_checkpoint(ck2)
    assert torch.load(ck2, weights_only=False)["ema"]["n_averaged"] == 1
