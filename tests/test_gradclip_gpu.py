"""Gradient clipping by the global norm (include/polyphemus_hip.h, "gradient clipping by the global norm"): the deterministic
double-precision sum of squares of the flat gradient, alone and in the read of the non-finite check; the finish
(norm = |grad_scale| sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)), gscale = float32(grad_scale coef)); Adam with the scale
read from the device; and `HipTrainer(..., max_grad_norm=...)` with its history of (norm, coef) rows."""
import math

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd.model import VAE
from polyphemus_amd.synthetic import synthetic_batch
from polyphemus_amd.trainer import HipTrainer
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
LR, BETAS, EPS = 1e-3, (0.9, 0.98), 1e-9
FMAX = float(np.finfo(np.float32).max)
# double accumulation of n non-negative terms: relative error <= n * 2^-53 = 1.2e-9 at n = 10.8 M (far below at the small sizes)
TOL = 1e-9
SIZES = [1, 3, 4, 4096, 4097, 10_800_000]


def _f32(x) -> float:
    return float(np.float32(x))


def _rand(n, offset, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n + offset, device=DEV, generator=g)[offset:]


def _measure(x, clip=None, max_norm=INF, grad_scale=1.0):
    """stand-alone pass + finish; the clip block (device)"""
    clip = ops.clip_block(DEV) if clip is None else clip
    ops.grad_sumsq(x, clip)
    ops.grad_clip_finish(clip, max_norm, grad_scale)
    return clip


def _ref_sumsq(x) -> float:
    """numpy on the host: float32 -> float64 keeps denormals whatever the device's conversion does"""
    return float((x.cpu().numpy().astype(np.float64) ** 2).sum())


def _coef(max_norm, norm) -> float:
    """the header's formula in Python doubles; fmin(1.0, NaN) = 1.0"""
    q = _f32(max_norm) / (norm + 1e-6) if not (math.isinf(max_norm) and math.isinf(norm)) else float("nan")
    return 1.0 if math.isnan(q) else min(1.0, q)


def _close(a, b, tol=TOL):
    return abs(a - b) <= tol * abs(b)


# ---------------------------------------------------------------------------------------------- sum of squares
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1])
def test_sumsq_matches_double_reference_and_is_deterministic(n, offset):
    """Aligned (uint4 kernel, at 10.8 M its four-loads-in-flight loop and the tail) and offset by one element (scalar kernel):
    the sum of squares is within 1e-9 of `x.double().pow(2).sum()`, norm = sqrt of it, and a second call gives equal bits."""
    x = _rand(n, offset, 11 * n + offset)
    ref = float(x.double().pow(2).sum())
    a = _measure(x).clone()
    b = _measure(x)
    assert torch.equal(a, b), "two runs on the same gradient differ"
    got = a.tolist()
    print(f"n={n} offset={offset} rel={abs(got[ops.CLIP_SUMSQ] - ref) / ref:.3e}")
    assert _close(got[ops.CLIP_SUMSQ], ref)
    assert _close(got[ops.CLIP_NORM], math.sqrt(ref))
    assert got[ops.CLIP_COEF] == 1.0 and got[ops.CLIP_GSCALE] == 1.0
    # sumsq is the sum of the partials in slot order
    s = 0.0
    for v in got[ops.CLIP_PARTIALS_AT:ops.CLIP_PARTIALS_AT + ops.CLIP_PARTIALS]:
        s += v
    assert s == got[ops.CLIP_SUMSQ]


@pytest.mark.parametrize("fused", [False, True])
def test_smaller_launch_after_a_larger_one_reads_no_stale_partials(fused):
    """n = 4096 (one workgroup) after 10.8 M (256 workgroups) on the SAME block gives the small buffer's value."""
    big, small = _rand(10_800_000, 0, 1), _rand(4096, 0, 2)
    fresh = _measure(small).clone()
    clip = ops.clip_block(DEV)
    status = ops.overflow_status(DEV)
    for x in (big, small):
        if fused:
            ops.grad_nonfinite_check_sumsq(x, status, clip)
        else:
            ops.grad_sumsq(x, clip)
        ops.grad_clip_finish(clip, INF)
    assert torch.equal(clip, fresh)
    assert _close(float(clip[ops.CLIP_SUMSQ]), _ref_sumsq(small))


@pytest.mark.parametrize("offset", [0, 1])
def test_sumsq_at_the_edges_of_fp32(offset):
    """Squares formed in fp32 would overflow at |g| > 1.8e19 and vanish below 1e-23: +-1e30, +-1e-30, denormals, one FLT_MAX
    among ones all give the finite, non-zero double result; all zeros give norm 0, coef 1.0, no NaN."""
    n = 4099
    sign = torch.where(torch.arange(n + offset, device=DEV) % 3 == 0, -1.0, 1.0)
    den = torch.tensor([1e-45, -1e-40, 3e-39, -1.1e-38], device=DEV).repeat((n + offset + 3) // 4)[:n + offset]
    assert float(den.abs().max()) < float(np.finfo(np.float32).tiny) and float(den.abs().min()) > 0
    ones = torch.ones(n + offset, device=DEV)
    ones[offset + n // 2] = FMAX
    for name, buf in (("1e30", sign * 1e30), ("1e-30", sign * 1e-30), ("denormals", den), ("FLT_MAX", ones)):
        x = buf[offset:]
        ref = _ref_sumsq(x)
        assert ref > 0 and math.isfinite(ref)
        got = _measure(x, max_norm=1.0).tolist()
        assert math.isfinite(got[ops.CLIP_NORM]) and got[ops.CLIP_NORM] > 0, name
        assert _close(got[ops.CLIP_SUMSQ], ref), (name, got[ops.CLIP_SUMSQ], ref)
        assert _close(got[ops.CLIP_NORM], math.sqrt(ref)), name
        assert got[ops.CLIP_COEF] == _coef(1.0, got[ops.CLIP_NORM]), name
    got = _measure(torch.zeros(n + offset, device=DEV)[offset:], max_norm=1.0, grad_scale=0.5).tolist()
    assert got[ops.CLIP_SUMSQ] == 0.0 and got[ops.CLIP_NORM] == 0.0 and got[ops.CLIP_COEF] == 1.0 and got[ops.CLIP_GSCALE] == 0.5


def test_finish_scales_the_norm_and_records_the_row():
    """norm is that of grad_scale * grads (|grad_scale|: a negative scale too), coef and gscale follow the formula, the row
    receives (norm, coef)."""
    x = _rand(4097, 0, 3)
    ref = math.sqrt(_ref_sumsq(x))
    for gs, mx in ((0.5, INF), (-0.25, 1.0), (1.0, 3.0), (1.0, 1e9)):
        clip, row = ops.clip_block(DEV), torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
        ops.grad_sumsq(x, clip)
        ops.grad_clip_finish(clip, mx, gs, row)
        got = clip.tolist()
        assert _close(got[ops.CLIP_NORM], abs(gs) * ref)
        assert got[ops.CLIP_COEF] == _coef(mx, got[ops.CLIP_NORM])
        assert got[ops.CLIP_GSCALE] == _f32(gs * got[ops.CLIP_COEF])
        assert row.tolist() == [got[ops.CLIP_NORM], got[ops.CLIP_COEF]]


# ---------------------------------------------------------------------------------------------- fused with the check
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1])
def test_fused_check_gives_the_same_sums_and_the_same_flag(n, offset):
    """One read of the gradient: the partials equal the stand-alone pass bit for bit; the flag equals `grad_nonfinite_check` for
    NaN / +-inf and for finite extremes at the first, a middle and the last position."""
    x = _rand(n, offset, 7 * n + offset)
    st_a, st_b = ops.overflow_status(DEV), ops.overflow_status(DEV)
    clip = ops.clip_block(DEV)
    ops.grad_nonfinite_check_sumsq(x, st_a, clip)
    ops.grad_clip_finish(clip, INF)
    assert torch.equal(clip, _measure(x))
    assert int(st_a[ops.OVF_PENDING]) == 0
    for v in (FMAX, -FMAX, 1e-45, -0.0, float("nan"), INF, -INF):
        for pos in sorted({0, n // 2, n - 1}):
            st_a.zero_(); st_b.zero_()
            keep = x[pos].clone()
            x[pos] = v
            ops.grad_nonfinite_check_sumsq(x, st_a, clip)
            ops.grad_nonfinite_check(x, st_b)
            ops.grad_clip_finish(clip, INF)
            alone = _measure(x)
            x[pos] = keep
            assert torch.equal(st_a, st_b), (v, pos)
            assert int(st_a[ops.OVF_PENDING]) == (0 if math.isfinite(v) else ops.OVF_NONFINITE_BIT), (v, pos)
            assert torch.equal(clip.view(torch.int64), alone.view(torch.int64)), (v, pos)     # (bits: NaN == NaN)


@pytest.mark.parametrize("n,offset", [(4099, 0), (4096, 1), (10_800_000, 0)])
def test_fused_check_decides_as_the_check_alone(n, offset):
    """With the step / skipped words the fused launch DECIDES like `grad_nonfinite_check`: same status block, same counts, for
    a finite gradient, a NaN in it and a pending cause; the ticket is back at 0."""
    x = _rand(n, offset, 21)
    clip = ops.clip_block(DEV)
    st_a, st_b = ops.overflow_status(DEV), ops.overflow_status(DEV)
    cnt_a, cnt_b = (torch.tensor([4, 1], dtype=torch.int64, device=DEV) for _ in range(2))
    for case in ("finite", "nan", "pending", "finite"):
        keep = x[n // 2].clone()
        if case == "nan":
            x[n // 2] = float("nan")
        if case == "pending":
            st_a[ops.OVF_PENDING] = ops.OVF_SATURATED_BIT
            st_b[ops.OVF_PENDING] = ops.OVF_SATURATED_BIT
        ops.grad_nonfinite_check_sumsq(x, st_a, clip, cnt_a[0:1], cnt_a[1:2], LR, *BETAS)
        ops.grad_nonfinite_check(x, st_b, cnt_b[0:1], cnt_b[1:2], LR, *BETAS)
        x[n // 2] = keep
        assert torch.equal(st_a, st_b) and torch.equal(cnt_a, cnt_b), case
        assert int(st_a[ops.OVF_TICKET]) == 0
        assert (int(st_a[ops.OVF_LAST]) != 0) == (case != "finite")
    assert cnt_a.tolist() == [6, 3]


# ---------------------------------------------------------------------------------------------- clipped Adam
def _adam_buffers(n, offset, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    mk = lambda: torch.randn(n + offset, device=DEV, generator=g)[offset:]
    p, m = mk(), mk() * 1e-3
    v = mk().abs() * 1e-6
    return p, m, v, g


@pytest.mark.parametrize("n,offset", [(8192, 0), (4099, 0), (4096, 1), (1, 0), (3, 1), (4, 0)])
@pytest.mark.parametrize("guard", [False, True])
@pytest.mark.parametrize("mode", ["inf", "x10"])
def test_unclipped_adam_equals_adam_step_bitwise(n, offset, guard, mode):
    """max_norm = inf, and max_norm ten times the norm: coef == 1.0, gscale == grad_scale, and over three steps the parameters
    and both moments equal `ops.adam_step` bit for bit (float4 and scalar kernel; host scalars and the guarded step's)."""
    p, m, v, g = _adam_buffers(n, offset, 5)
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    clip, row = ops.clip_block(DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    status = ops.overflow_status(DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in range(1, 4):
        grad = torch.randn(n + offset, device=DEV, generator=g)[offset:]
        mx = INF if mode == "inf" else 10.0 * 0.5 * float(grad.double().norm())
        if guard:
            ops.grad_nonfinite_check_sumsq(grad, status, clip, cnt[0:1], cnt[1:2], LR, *BETAS)
        else:
            ops.grad_sumsq(grad, clip)
        ops.grad_clip_finish(clip, mx, 0.5, row)
        ops.adam_step_clipped(p, grad, m, v, LR, *BETAS, EPS, t, clip, status if guard else None)
        ops.adam_step(rp, grad, rm, rv, LR, *BETAS, EPS, t, grad_scale=0.5)
        assert row.tolist()[1] == 1.0 and float(clip[ops.CLIP_GSCALE]) == 0.5
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), t
    if guard:
        assert cnt.tolist() == [3, 0]


@pytest.mark.parametrize("n,offset", [(8192, 0), (4099, 0), (4096, 1)])
@pytest.mark.parametrize("guard", [False, True])
def test_clipped_adam_equals_adam_step_at_the_recomputed_scale_and_torch(n, offset, guard):
    """max_norm half the norm, three steps: bitwise equal to `ops.adam_step` called with grad_scale = float32(grad_scale * coef),
    coef recomputed in Python doubles from the recorded norm; the recorded coef is that value; and within 1e-6 of
    `clip_grad_norm_` + `torch.optim.Adam` on a copy (the bound of test_adam_matches_torch)."""
    gs = 0.5
    p = _rand(n, offset, 17)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    rp, rm, rv = p.clone(), m.clone(), v.clone()
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS)
    clip, row = ops.clip_block(DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
    status = ops.overflow_status(DEV)
    cnt = torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in range(1, 4):
        grad = _rand(n, offset, 100 + t)
        mx = _f32(0.5 * gs * float(grad.double().norm()))
        if guard:
            ops.grad_nonfinite_check_sumsq(grad, status, clip, cnt[0:1], cnt[1:2], LR, *BETAS)
        else:
            ops.grad_sumsq(grad, clip)
        ops.grad_clip_finish(clip, mx, gs, row)
        ops.adam_step_clipped(p, grad, m, v, LR, *BETAS, EPS, t, clip, status if guard else None)
        norm, coef = row.tolist()
        assert _close(norm, gs * float(grad.double().norm()))
        want = _coef(mx, norm)
        assert coef == want and 0.49 < coef < 0.51
        ops.adam_step(rp, grad, rm, rv, LR, *BETAS, EPS, t, grad_scale=_f32(gs * want))
        assert torch.equal(p, rp) and torch.equal(m, rm) and torch.equal(v, rv), t
        tp.grad = grad * gs
        tn = torch.nn.utils.clip_grad_norm_([tp], mx)
        assert _close(norm, float(tn), 1e-5)                           # (torch's norm is a float32 reduction)
        opt.step()
        assert rel_err(p, tp.detach()) < 1e-6


@pytest.mark.parametrize("cause", [ops.OVF_NONFINITE_BIT, ops.OVF_SATURATED_BIT])
def test_guarded_clipped_adam_skipped_stores_nothing_and_records_the_norm(cause):
    for n, offset in ((8192, 0), (4097, 1)):
        p, m, v, g = _adam_buffers(n, offset, 9)
        grad = torch.randn(n + offset, device=DEV, generator=g)[offset:]
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        clip, row = ops.clip_block(DEV), torch.zeros(2, dtype=torch.float64, device=DEV)
        status = ops.overflow_status(DEV)
        cnt = torch.tensor([7, 2], dtype=torch.int64, device=DEV)
        status[ops.OVF_PENDING] = cause
        ops.grad_nonfinite_check_sumsq(grad, status, clip, cnt[0:1], cnt[1:2], LR, *BETAS)
        ops.grad_clip_finish(clip, 1.0, 1.0, row)
        ops.adam_step_clipped(p, grad, m, v, LR, *BETAS, EPS, 0, clip, status)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert cnt.tolist() == [7, 3] and int(status[ops.OVF_LAST]) == cause
        norm, coef = row.tolist()
        assert _close(norm, float(grad.double().norm())) and coef == _coef(1.0, norm)
        # a NaN in the gradient: skipped by the check itself, the recorded norm is NaN
        grad[n // 3] = float("nan")
        ops.grad_nonfinite_check_sumsq(grad, status, clip, cnt[0:1], cnt[1:2], LR, *BETAS)
        ops.grad_clip_finish(clip, 1.0, 1.0, row)
        ops.adam_step_clipped(p, grad, m, v, LR, *BETAS, EPS, 0, clip, status)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert cnt.tolist() == [7, 4] and math.isnan(row.tolist()[0]) and row.tolist()[1] == 1.0


def test_nonfinite_gradient_under_ignore_follows_ieee():
    """No special case: an inf in the gradient gives norm = inf, coef = max / inf = 0 (max_norm = inf: fmin(1, NaN) = 1); a NaN
    gives norm = NaN and coef = fmin(1, NaN) = 1.  Adam then consumes the non-finite values, as after torch's clip."""
    x = _rand(4096, 0, 4)
    x[17] = INF
    got = _measure(x, max_norm=2.0).tolist()
    assert got[ops.CLIP_NORM] == INF and got[ops.CLIP_COEF] == 0.0 and got[ops.CLIP_GSCALE] == 0.0
    got = _measure(x, max_norm=INF).tolist()
    assert got[ops.CLIP_NORM] == INF and got[ops.CLIP_COEF] == 1.0 and got[ops.CLIP_GSCALE] == 1.0
    x[17] = float("nan")
    got = _measure(x, max_norm=2.0).tolist()
    assert math.isnan(got[ops.CLIP_NORM]) and got[ops.CLIP_COEF] == 1.0 and got[ops.CLIP_GSCALE] == 1.0


# ---------------------------------------------------------------------------------------------- trainer
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)     # tests/test_overflow_gpu.py


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


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("overflow", ["ignore", "skip"])
def test_trainer_measures_with_inf_and_clips_below_the_norm(native, overflow):
    """Deterministic mode.  max_grad_norm = inf over three steps: parameters and moments bitwise equal to a trainer built
    without the option from the same seed; three rows, each norm within 1e-9 of `tr.grads.double().norm()` after that step,
    each coef 1.0.  Then max_grad_norm = half the first norm: after each step the parameters equal `ops.adam_step` of the
    pre-update state with `tr.grads` at the scale float32(coef) recomputed from the recorded norm, bit for bit; coef < 1."""
    with _lib.deterministic(True):
        plain = HipTrainer(_model(), lr=LR, native=native, overflow=overflow)
        tr = HipTrainer(_model(), lr=LR, native=native, overflow=overflow, max_grad_norm=INF)
        norms = []
        for k in range(1, 4):
            plain.train_step(*_batch(50 + k))
            tr.train_step(*_batch(50 + k))
            norms.append(float(tr.grads.double().norm()))
            assert float(tr.last_grad_norm) > 0
            for a, b in zip(_state(tr), _state(plain)):
                assert torch.equal(a, b), k
        rows = tr.read_grad_norms()
        assert len(rows) == 3 and tr.read_grad_norms() == []
        for (norm, coef), ref in zip(rows, norms):
            assert _close(norm, ref) and coef == 1.0
        assert tr.step_count == plain.step_count == 3

        mx = rows[0][0] / 2
        tr = HipTrainer(_model(), lr=LR, native=native, overflow=overflow, max_grad_norm=mx)
        for k in range(1, 4):
            p0, m0, v0 = _state(tr)
            tr.train_step(*_batch(50 + k))
            (norm, coef), = tr.read_grad_norms()
            assert _close(norm, float(tr.grads.double().norm())) and norm == float(tr.last_grad_norm)
            want = _coef(mx, norm)
            assert coef == want and coef < 1
            ops.adam_step(p0, tr.grads, m0, v0, LR, *BETAS, EPS, k, grad_scale=_f32(want))
            assert torch.equal(tr.vae.flat_params, p0) and torch.equal(tr.exp_avg, m0) and torch.equal(tr.exp_avg_sq, v0), k
        if overflow == "skip":
            assert int(tr.skipped_steps) == 0


def test_trainer_accumulation_records_one_row_per_update():
    """iters_to_accumulate = 2: micro-batches that do not update record nothing; the norm is that of `tr.grad_accum`."""
    tr = HipTrainer(_model(), lr=LR, iters_to_accumulate=2, max_grad_norm=INF)
    for pair in range(2):
        tr.train_step(*_batch(40 + 2 * pair))
        assert tr.read_grad_norms() == []
        tr.train_step(*_batch(41 + 2 * pair))
        ref = float(tr.grad_accum.double().norm())
        (norm, coef), = tr.read_grad_norms()
        assert _close(norm, ref) and coef == 1.0
    assert tr.step_count == 2


def test_trainer_skip_records_the_nonfinite_norm_of_a_skipped_update():
    """overflow="skip" with a NaN written into the accumulated gradient (as test_trainer_skips_a_nonfinite_accumulated_gradient):
    state unchanged, the row is recorded with a non-finite norm."""
    tr = HipTrainer(_model(), lr=LR, iters_to_accumulate=2, overflow="skip", max_grad_norm=1.0)
    p0, m0, v0 = _state(tr)
    tr.train_step(*_batch(40))
    tr.grad_accum[12345] = float("nan")
    tr.train_step(*_batch(41))
    for a, b in zip(_state(tr), (p0, m0, v0)):
        assert torch.equal(a, b)
    assert tr.step_count == 0 and int(tr.skipped_steps) == 1
    (norm, coef), = tr.read_grad_norms()
    assert not math.isfinite(norm)


def test_trainer_history_capacity_and_feature_off():
    tr = HipTrainer(_model(), lr=LR, max_grad_norm=INF, grad_norm_capacity=2)
    tr.train_step(*_batch(60))
    tr.train_step(*_batch(61))
    p0 = tr.vae.flat_params.detach().clone()
    with pytest.raises(RuntimeError, match="gradient-norm history is full"):
        tr.train_step(*_batch(62))
    assert torch.equal(tr.vae.flat_params, p0) and tr.step_count == 2
    assert len(tr.read_grad_norms()) == 2
    tr.train_step(*_batch(62))
    assert len(tr.read_grad_norms()) == 1
    off = HipTrainer(_model(), lr=LR)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        off.read_grad_norms()
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        off.last_grad_norm
