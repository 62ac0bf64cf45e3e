"""Sync-free training step of the HIP graph-VAE (the measured hot path).

Mirrors one iteration of `PolyphemusTrainer.train` (reference training.py:129-172):
forward, `_losses`, backward, `optimizer.step()`, `zero_grad()`, `lr_scheduler.step()` —
but without autograd bookkeeping and without the reference's 7 `.item()` host syncs:

    plan build -> encoder -> reparametrisation -> decoder -> fused CE/KLD/BCE loss (+ dlogits)
    -> decoder backward -> reparam backward -> encoder backward
    -> [data parallel: RCCL all-reduce of the flat gradient in three buckets, two of them overlapped
        with the encoder backward] -> fused Adam on the flat parameter buffer

Two orchestrations of the SAME kernels:
  * native (default): four C calls (`pm_vae_step_forward`, `..._backward_decoder`,
    `..._backward_encoder`, `..._backward_encoder_tail`, csrc/vae_step.hip) issue the ~340 launches of a step from C++;
  * python (`native=False`): the same sequence through `engine.Engine` (the executable
    specification the autograd drop-in path uses); kept for cross-checking.

Reference quirks reproduced by default: the structure BCE is evaluated on the
target (no gradient reaches the structure decoder, B-1), beta stays 0 (B-3), message dropout
p = 0.1 is always on in training (B-2).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import warnings
from typing import Dict, Optional

import torch

from . import ops
from ._lib import call, h2_clamp_init, lib, ptr, stream
from .model import VAE, prepare_graph
from .native import NativeStep, prepare_inputs
from .parallel import GradBuckets, broadcast_


class ExpDecayLR:
    """`ExpDecayLRScheduler` (training.py:43-75): peak_lr during warm-up, then exponential decay."""

    def __init__(self, peak_lr, warmup_steps, final_lr_scale, decay_steps):
        self.peak_lr, self.warmup_steps = peak_lr, warmup_steps
        self.decay_factor = -math.log(final_lr_scale) / decay_steps
        self.update_steps = 0

    def step(self) -> float:
        self.update_steps += 1
        if self.update_steps <= self.warmup_steps:
            return self.peak_lr
        return self.peak_lr * math.exp(-self.decay_factor * (self.update_steps - self.warmup_steps))


def bucket_boundaries(vae: VAE):
    """Element offsets that split the flat gradient buffer into the three exchange buckets, in flat order: 0 = structure encoder
    + embeddings + chord encoder (final last: behind `pm_vae_step_backward_encoder_tail`), 1 = graph encoder .. end of the
    encoder (final behind `pm_vae_step_backward_encoder`), 2 = decoder (final behind the decoder backward and the join of its
    weight gradients).  Asserts the parameter order the native split relies on."""
    dec_lo = vae._offsets[vae._names("decoder.")[0]]
    mid_lo = vae._offsets[vae._names("encoder.c_encoder.graph_encoder.")[0]]
    for n in vae._names("encoder."):
        late = n.startswith(("encoder.s_encoder.", "encoder.c_encoder.non_drums", "encoder.c_encoder.drums",
                             "encoder.c_encoder.dur_emb", "encoder.c_encoder.bn_", "encoder.c_encoder.chord_encoder"))
        assert (vae._offsets[n] < mid_lo) == late, f"unexpected parameter order at {n}"
    return [mid_lo, dec_lo]


class HipTrainer:
    def __init__(self, vae: VAE, lr=5e-6, betas=(0.9, 0.98), eps=1e-9, lr_scheduler: Optional[dict] = None,
                 structure_loss_on_logits: bool = False, beta: float = 0.0, process_group=None, native: bool = True,
                 iters_to_accumulate: int = 1, global_token_mean: bool = False, sync_bn: bool = False,
                 overflow: str = "ignore", train_metrics: bool = False, metrics_capacity: int = 1024,
                 max_grad_norm: Optional[float] = None, grad_norm_capacity: int = 1024, ema_decay: Optional[float] = None):
        if overflow not in ("ignore", "skip"):
            raise ValueError(f"overflow must be 'ignore' or 'skip', not {overflow!r}")
        if max_grad_norm is not None:
            # (it crosses the C ABI as a float: a positive value that rounds to 0.0f is rejected here, not inside a step)
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or \
                    not ctypes.c_float(max_grad_norm).value > 0:
                raise ValueError(f"max_grad_norm must be None, a positive number (as a float32) or float('inf'), "
                                 f"not {max_grad_norm!r}")
        if isinstance(grad_norm_capacity, bool) or not isinstance(grad_norm_capacity, int) or grad_norm_capacity < 1:
            raise ValueError(f"grad_norm_capacity must be a positive int, not {grad_norm_capacity!r}")
        # (the average's weight crosses the C ABI as float32(1 - ema_decay): rejected here, not inside a step)
        self._ema_w = None if ema_decay is None else ops.ema_weight(ema_decay)
        if not isinstance(train_metrics, bool):
            raise ValueError(f"train_metrics must be True or False, not {train_metrics!r}")
        if train_metrics and (not isinstance(metrics_capacity, int) or metrics_capacity < 1):
            raise ValueError(f"metrics_capacity must be a positive int, not {metrics_capacity!r}")
        self.vae = vae
        self.lr, self.betas, self.eps = lr, betas, eps
        self.sched = ExpDecayLR(**lr_scheduler) if lr_scheduler else None
        self.fix_structure_loss = structure_loss_on_logits
        self.beta = beta
        self.pg = process_group
        # Data parallel: the reference's CE losses are means over the non-PAD tokens of the batch (training.py:316-323),
        # so the mean of per-rank gradients weights every rank equally whatever its token count.  With
        # `global_token_mean` each rank's CE gradient is weighted n_local * world / n_global (one all-reduce of two
        # counts per step, no host sync): the averaged gradient is then that of the token mean over the GLOBAL batch.
        self.global_token_mean = bool(global_token_mean)
        # True: the native step also stores the content logits (`step_outputs`); off by default — the fused un-embedding +
        # cross-entropy then writes d(loss)/d(logits) only
        self.keep_logits = False
        # the C++ step covers every constructor switch of the model (batch_norm = False: model.py:176-188,218-238,278-292;
        # cfg.dropout: the element dropout layers of model.py:160,199,244-247,267-270,389-390,473,479,558-559,640);
        # `native=False` selects the Python orchestration of the same kernels (engine.py), kept for cross-checking
        self.sync_bn = bool(sync_bn)
        import torch.distributed as _dist
        _world = _dist.get_world_size(process_group) if (_dist.is_available() and _dist.is_initialized()) else 1
        # Synchronised BatchNorm: every training-mode norm takes its statistics over the GLOBAL batch, so that
        # — together with global_token_mean — a data-parallel step equals the single-device step on the concatenated
        # batch.  Runs through the Python orchestration (one small all-reduce per norm and direction, one host read per
        # step); an option for parity checks, not for throughput runs.  With ONE rank the statistics are global anyway:
        # the native step stays on.
        self.native = bool(native and not (self.sync_bn and _world > 1))
        if iters_to_accumulate < 1:
            raise ValueError("iters_to_accumulate must be >= 1")
        self.iters_to_accumulate = int(iters_to_accumulate)            # training.py:83,149,158
        self.micro_batches = 0                                         # `tot_batches` of the reference
        flat = vae.flat_params
        if not flat.is_cuda:
            raise RuntimeError("HipTrainer needs the model on the GPU (vae.to('cuda')) before it is built")
        self.grads = torch.zeros_like(flat)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        # Overflow policy of the optimizer step.  "ignore": Adam applies whatever gradient it gets (no extra launch).
        # "skip": the reference's GradScaler semantics (training.py:123,152-162) — an update whose gradient holds an inf or
        # a NaN, or whose step saturated a split of the fp16 pair format on any rank, is skipped ON THE DEVICE (parameters,
        # moments and Adam's step count unchanged; the LR schedule still steps): a snapshot of the saturation counter, one read
        # of the gradient that also decides, no host sync.
        self.overflow = overflow
        self._guard = overflow == "skip"
        h2_clamp_init()                          # the saturation counter exists before any step reads it
        if self._guard:
            self._ovf_status = ops.overflow_status(flat.device)
            self._ovf_counts = torch.zeros(2, dtype=torch.int64, device=flat.device)     # [Adam's step count t, skipped]
            self._ovf_host = torch.zeros(1, dtype=torch.int64).pin_memory()             # skipped, copied without a sync
            self._ovf_event = torch.cuda.Event()
            self._ovf_copied = False
            self._ovf_warned = 0
        self.step_count = 0
        # Clipping by the global norm (what `torch.nn.utils.clip_grad_norm_` in front of `optimizer.step()` gives the
        # reference loop; the reference itself does not clip).  None: nothing of it runs.  A number: the gradient Adam
        # consumes — the mean over ranks, or the accumulated one — is scaled by min(1, max / (norm + 1e-6)) on the device;
        # inf: measured only.  One (norm, coef) row per optimizer update goes into a device history of `grad_norm_capacity`
        # rows; `read_grad_norms` takes them with one sync.
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None:
            self._clip = ops.clip_block(flat.device)
            self._nhist = torch.zeros(grad_norm_capacity, 2, dtype=torch.float64, device=flat.device)
            self._nrows = 0                       # rows written since the last read (host count)
        self.loss_buf = torch.zeros(4, dtype=torch.float64, device=flat.device)
        # Training accuracies (the reference's `_accuracies` after every batch, training.py:174-179): one int64 counts row per
        # batch (ops.accuracies_from_counts has the layout), written by the step on the device into a history of
        # `metrics_capacity` rows; `read_train_accuracies` takes them with one sync.  Off: nothing of it runs.
        self.train_metrics = train_metrics
        self._mhist = torch.zeros(metrics_capacity, 16, dtype=torch.int64, device=flat.device) if train_metrics else None
        self._mrows = 0                           # rows written since the last read (host count: no sync decides anything)
        P = dict(vae.named_parameters())
        self._G: Dict[str, torch.Tensor] = {}
        for n in vae._param_names:
            o = vae._offsets[n]
            self._G[n] = self.grads[o:o + P[n].numel()].view(P[n].shape)
        for k in list(self._G):
            if ".layers.0.nn." in k:
                head, tail = k.split(".layers.0.nn.")
                for i in range(1, vae.cfg["gnn_n_layers"]):
                    self._G[f"{head}.layers.{i}.nn.{tail}"] = self._G[k]
        self.buckets = GradBuckets(self.grads, bucket_boundaries(vae), process_group)
        self.world = self.buckets.world
        # the +inf that carries a saturation is needed only where the gradient travels (an exchange, an accumulation); a
        # single-rank step gets the verdict from the check itself, which compares the counter with the snapshot
        self._poison = self._guard and (self.world > 1 or self.iters_to_accumulate > 1)
        # gradient accumulation: running sum of grads / k; all-reduced (one bucket) and consumed by Adam every k-th batch
        self.grad_accum = torch.zeros_like(flat) if self.iters_to_accumulate > 1 else None
        self._accum_bucket = GradBuckets(self.grad_accum, [], process_group) if self.grad_accum is not None else None
        broadcast_([vae.flat_params, vae.flat_buffers], 0, process_group)
        # Exponential moving average of the parameters (what `torch.optim.swa_utils.AveragedModel` with
        # `get_ema_multi_avg_fn(ema_decay)`, updated behind every `optimizer.step()`, gives the reference loop; the reference
        # itself keeps none).  None: nothing of it runs.  A decay in [0, 1): `self.ema`, a flat buffer like the moments, starts
        # as a copy of the (broadcast) initial weights — AveragedModel's first update copies too — and every APPLIED optimizer
        # update moves it inside the Adam launch: ema += (1 - decay) * (p - ema).  An update the guard skips leaves it alone.
        # Parameters only: BatchNorm's running statistics stay the live model's (AveragedModel(use_buffers=False)).
        # `ema_weights()`, `evaluate*(ema=True)`, `ema_state_dict()` and the checkpoint use it.
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema = flat.detach().clone() if self._ema_w is not None else None
        self._ema_t0 = 0                                   # Adam's t when the average started (n_averaged = t - t0)
        self._ema_swapped = False                          # inside `ema_weights()`: flat_params holds the average
        vae.engine.set_sync_bn(process_group, self.sync_bn and self.world > 1)
        # every rank its own message-dropout stream (same seed = same masks on every replica): the model keeps its BASE
        # seed — what checkpoints store — and the rank only salts the seeds derived from it (VAE._next_seed), so building a
        # second trainer on the same model, resuming from a rank-0 checkpoint or resuming with another world size all give
        # each rank a stream of its own
        vae.rank_salt = 0
        if self.world > 1:
            import torch.distributed as dist
            vae.rank_salt = (0x9E3779B9 * (dist.get_rank(process_group) + 1)) & 0xFFFFFFFF
        # native step plumbing (polyphemus_amd/native.py: layout, host state blob, arena, plan buffer)
        self._flat_ptr = flat.data_ptr()
        self.step = NativeStep(vae) if self.native else None
        self.loss_buf = self.step.loss_buf if self.step is not None else self.loss_buf

    # ------------------------------------------------------------------------------------------
    @property
    def _plan_buf(self):
        return self.step.plan_buf

    @property
    def step_count(self) -> int:
        """Adam's step count t.  With overflow="skip" it lives on the device (a skipped step does not advance it): reading
        it then synchronises."""
        return int(self._ovf_counts[0]) if self._guard else self._step_count

    @step_count.setter
    def step_count(self, t: int) -> None:
        self._step_count = int(t)
        if self._guard:
            self._ovf_counts[0].fill_(int(t))

    @property
    def skipped_steps(self) -> torch.Tensor:
        """Device int64 count of the optimizer steps skipped on a non-finite or saturated gradient (overflow="skip")."""
        return self._ovf_counts[1] if self._guard else torch.zeros((), dtype=torch.int64, device=self.grads.device)

    @property
    def last_update_skipped(self) -> torch.Tensor:
        """Device bool: the last optimizer step was skipped (overflow="skip")."""
        if not self._guard:
            return torch.zeros((), dtype=torch.bool, device=self.grads.device)
        return self._ovf_status[ops.OVF_LAST] != 0

    def overflow_stats(self) -> dict:
        """Host dict of the guard's counters (this DOES sync): skipped optimizer steps, and of them those with a saturated
        pair-format split on this rank (`saturated`) and the others (`non_finite`: an inf / NaN gradient, or a saturation on
        another rank that reached this one through the all-reduce)."""
        if not self._guard:
            return {"skipped": 0, "non_finite": 0, "saturated": 0}
        st = self._ovf_status.tolist()
        return {"skipped": int(self._ovf_counts[1]), "non_finite": st[ops.OVF_N_NONFINITE],
                "saturated": st[ops.OVF_N_SATURATED]}

    def _warn_skips(self) -> None:
        """RuntimeWarning for steps skipped since the last warning, read from the copy the previous step made — only if it
        has arrived (event query, never a wait)."""
        if not (self._ovf_copied and self._ovf_event.query()):
            return
        self._ovf_copied = False
        n = int(self._ovf_host[0])
        if n > self._ovf_warned:
            warnings.warn(f"{n - self._ovf_warned} optimizer step(s) skipped on a non-finite or saturated gradient ({n} so "
                          "far; trainer.overflow_stats() has the causes)", RuntimeWarning, stacklevel=3)
            self._ovf_warned = n

    def _native_forward_backward(self, graph, eps):
        vae, step = self.vae, self.step
        ce_scale = None
        gtm = self.global_token_mean and self.world > 1
        if gtm:
            import torch.distributed as dist
            inputs = prepare_inputs(graph, want_token_counts=True)
            tot = inputs[9].clone()
            dist.all_reduce(tot, group=self.pg)
            ce_scale = (inputs[9] * float(self.world) / tot).contiguous()      # stays on the device
        if self._guard:                                      # in front of the prologue's weight-plane splits
            call("pm_overflow_snapshot", self._ovf_status.data_ptr(), stream())
        if self.train_metrics:                               # arm the step on this batch's row (host pointer arithmetic)
            call("pm_vae_step_set_metrics", step.addr, self._mhist[self._mrows].data_ptr())
        step.forward(graph, eps, self.grads, keep_logits=self.keep_logits, beta=self.beta,
                     fix_structure=self.fix_structure_loss, ce_scale=ce_scale, want_token_counts=gtm)
        if prepare_inputs(graph)[8] and os.environ.get("PM_DEBUG", "0") not in ("", "0"):
            # the plan kernels count the nodes that break the one-track-relation-per-node rule the compact GCL
            # relies on (plan.hip k_node_class, cnt[4]); a host read, hence only under PM_DEBUG
            bad = step.plan_word("trk_cnt", 4)
            if bad:
                raise RuntimeError(f"{bad} nodes receive track edges of more than one track but the batch was "
                                   "flagged track_unique (graphs.batch_flags); the compact GCL would be wrong")
        step.backward_decoder()
        # the decoder's last weight gradients run on the library's second stream beside the head chains; the encoder's head
        # chain ends with the caller's stream waiting for them, so the decoder bucket goes out behind it — in front of the
        # encoder's GCN stack, which overlaps the exchange
        step.backward_encoder_heads()
        self.buckets.launch(2)                               # decoder gradients: overlapped with the encoder backward
        step.backward_encoder()
        self.buckets.launch(1)                               # graph encoder .. encoder head: overlapped with the tail
        step.backward_encoder_tail()
        if self._poison:                                     # every producer has joined: a saturation becomes +inf in bucket 0
            ops.overflow_poison(self.grads, self._ovf_status)
        self.buckets.launch(0)                               # chord encoder, embeddings, structure encoder
        step.bump_counters()
        return step.loss_buf

    @property
    def last_train_counts(self) -> torch.Tensor:
        """Device int64 [16] view of the latest batch's training-accuracy counts (layout: `ops.accuracies_from_counts`)."""
        if not self.train_metrics:
            raise RuntimeError("last_train_counts needs HipTrainer(..., train_metrics=True)")
        if self._mrows == 0:
            raise RuntimeError("no training-accuracy counts since the last read_train_accuracies()")
        return self._mhist[self._mrows - 1]

    def read_train_accuracies(self, reduce: bool = False) -> list:
        """One dict of the reference's 9 training accuracies (note, pitch, pitch_drums, pitch_non_drums, dur, s_acc,
        s_precision, s_recall, s_f1) per `train_step` since the last read, in order — what the reference appends to
        `tr_accuracies` after every batch (training.py:174-179).  Arg-max over the raw logits, the lowest index on ties.
        `reduce=True` first sums the counts over the trainer's process group: the accuracies one device would report on the
        concatenated batch.  One host sync; empties the history."""
        if not self.train_metrics:
            raise RuntimeError("read_train_accuracies needs HipTrainer(..., train_metrics=True)")
        rows = self._mhist[:self._mrows]
        if reduce and self.world > 1:
            import torch.distributed as dist
            rows = rows.clone()
            dist.all_reduce(rows, group=self.pg)
        host = rows.tolist()                               # the one sync
        self._mrows = 0
        return [ops.accuracies_from_counts(r) for r in host]

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Device float64 view of the norm of the gradient the last optimizer update consumed, before clipping (no sync)."""
        if self.max_grad_norm is None:
            raise RuntimeError("last_grad_norm needs HipTrainer(..., max_grad_norm=...)")
        return self._clip[ops.CLIP_NORM]

    def read_grad_norms(self) -> list:
        """`[(norm, coef), ...]`, one pair per optimizer update since the last read, in order: the global L2 norm of the
        gradient Adam consumed (a skipped update's too, possibly inf or NaN) and the factor it was scaled by,
        min(1, max_grad_norm / (norm + 1e-6)).  Every rank holds the same bits.  One host sync; empties the history."""
        if self.max_grad_norm is None:
            raise RuntimeError("read_grad_norms needs HipTrainer(..., max_grad_norm=...)")
        host = self._nhist[:self._nrows].tolist()          # the one sync
        self._nrows = 0
        return [(r[0], r[1]) for r in host]

    def step_info(self) -> dict:
        """Which variant of the native step the last `train_step` ran (`pm_vae_step_info`): compact GCL (K = 4d),
        bf16-planes GEMM operands, active token slots S, fragment-major weight planes (B-direct GEMM), batch sizes, the
        library's effective switches, the fp16 pair format of the GCL products (bit 0 encoder, bit 1 decoder stack)."""
        return self.step.info()

    def step_outputs(self):
        """`((s_logits, c_logits), mu, log_var)` of the last native `train_step` — what `VAE.forward` returns
        (model.py:676-678) — copied out of the workspace arena.  c_logits holds the active slots only: [N, S, 230]
        (the remaining slots are PAD in every node of the batch; the fused step never computes them)."""
        i = self.step_info()              # (the library's effective switches, not the environment at call time)
        if not self.keep_logits and i["fused_ce"]:
            raise RuntimeError("step_outputs needs trainer.keep_logits = True before the step (the fused un-embedding + "
                               "cross-entropy does not store the logits otherwise)")
        return self.step.outputs()

    def _python_forward_backward(self, graph, eps):
        vae, eng = self.vae, self.vae.engine
        if self._guard:
            ops.overflow_snapshot(self._ovf_status)
        eng.msg_dropout = vae.msg_dropout
        graph.__dict__.pop("_pm_plan", None)                 # the plan is part of the step (new batch every step)
        plan = prepare_graph(graph, vae.cfg["n_bars"])
        G = self._G
        s_tensor = graph.s_tensor.float().contiguous()
        mu, lv, esv = eng.encoder_forward(plan, s_tensor, True, vae._next_seed())
        if eps is None:
            eps = torch.randn_like(mu)
        z = ops.reparam_fwd(mu, lv, eps)
        s_logits, c_logits, dsv = eng.decoder_forward(plan, z, True, vae._next_seed())
        ce_scale = 1.0
        if self.global_token_mean and self.world > 1:          # weight n_local * world / n_global (a host read: this
            import torch.distributed as dist                   # orchestration is the parity path, not the measured one)
            tok = plan.tokens
            n_loc = (tok[:, 1:, 0] != 130).sum().double().reshape(1)
            n_all = n_loc.clone()
            dist.all_reduce(n_all, group=self.pg)
            ce_scale = float(n_loc.item()) * self.world / float(n_all.item())
        out, dc = ops.content_ce(c_logits, plan, grad_scale=ce_scale, want_grad=True, out=self.loss_buf)
        dmu, dlv = torch.zeros_like(mu), torch.zeros_like(lv)
        ops.kld(mu, lv, out, beta=self.beta, dmu=dmu, dlog_var=dlv)
        if self.fix_structure_loss:
            _, ds = ops.bce_logits(s_logits.reshape(-1), s_tensor.reshape(-1), out, 1.0, want_grad=True)
            ds = ds.view_as(s_logits)
        else:                                                # training.py:307: BCE of the target against itself
            ops.bce_logits(s_tensor.reshape(-1), s_tensor.reshape(-1), out, 1.0, want_grad=False)
            ds = None
        if self.train_metrics:                               # the same counts from this orchestration's own logits
            row = self._mhist[self._mrows]
            cl = c_logits.contiguous()
            row[:8].copy_(ops.content_accuracy(cl, plan.tokens, plan.is_drum) if cl.shape[1] == 15 else
                          ops.content_accuracy_slots(cl, plan.tokens, plan.is_drum)[:8])
            s_in = s_logits.reshape(-1).contiguous() if self.fix_structure_loss else s_tensor.reshape(-1)
            row[8:12].copy_(ops.structure_metrics(s_in, s_tensor.reshape(-1)))
            row[12].fill_(s_tensor.numel())
            row[13:].zero_()
        dz = eng.decoder_backward(dsv, ds, dc, G)
        self.buckets.launch(2)
        ops.reparam_bwd(dz, lv, eps, dmu, dlv)
        eng.encoder_backward(esv, dmu, dlv, G)
        self.buckets.launch(1)
        if self._poison:
            ops.overflow_poison(self.grads, self._ovf_status)
        self.buckets.launch(0)
        return out

    def _optimizer_update(self, grads, mean_scale):
        """The optimizer part of a step (training.py:160-166) in three stages: the read of the gradient that the options
        need, the finish of the clip, one Adam launch.  Raw `call`s throughout: the buffers are the trainer's own, made by
        its constructor, and the checks of the `ops` wrappers would be host work on every step."""
        guard, clip = self._guard, self.max_grad_norm is not None
        st, gp, n = stream(), grads.data_ptr(), grads.numel()
        b1, b2 = self.betas[0], self.betas[1]
        if guard:                                      # scaler.step(optimizer): no update on found_inf (training.py:160-162);
            sp, cp = self._ovf_status.data_ptr(), self._ovf_counts.data_ptr()      # the check decides t and its scalars
            decide = (sp, cp, cp + 8, self.lr, b1, b2, 1)
            lr, t = 0.0, 0
        else:
            self.step_count += 1
            sp, lr, t = None, self.lr, self.step_count
        if clip:                                       # this update's (norm, coef) row (host pointer arithmetic)
            kp, rp = self._clip.data_ptr(), self._nhist[self._nrows].data_ptr()
        # 1. the read of the gradient (with both options the check's read also takes the sum of squares)
        if guard and clip:
            call("pm_grad_nonfinite_check_sumsq", gp, n, *decide, kp, st)
        elif guard:
            call("pm_grad_nonfinite_check", gp, n, *decide, st)
        elif clip:
            call("pm_grad_sumsq", gp, n, kp, st)
        # 2. norm, coef and the gradient scale from the partial sums
        if clip:
            call("pm_grad_clip_finish", kp, mean_scale, self.max_grad_norm, rp, st)
        # 3. Adam: the scale from the clip block or `mean_scale`, t and its scalars from the decision or the host
        bufs = (self.vae.flat_params.data_ptr(), gp, self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n)
        if self._ema_w is not None:                    # the one entry for the four combinations, the average riding in it
            call("pm_adam_step_ema", *bufs[:4], self.ema.data_ptr(), n, lr, b1, b2, self.eps, t, mean_scale, self._ema_w,
                 kp if clip else None, sp, st)
        elif clip:
            call("pm_adam_step_clipped", *bufs, lr, b1, b2, self.eps, t, kp, sp, st)
        elif guard:
            call("pm_adam_step_guarded", *bufs, b1, b2, self.eps, mean_scale, sp, st)
        else:
            call("pm_adam_step", *bufs, lr, b1, b2, self.eps, t, mean_scale, st)
        if guard:
            self._ovf_host.copy_(self._ovf_counts[1:2], non_blocking=True)
            self._ovf_event.record()
            self._ovf_copied = True
        if clip:
            self._nrows += 1                               # (behind the launches: the count is of rows that were written)

    def train_step(self, graph, eps: Optional[torch.Tensor] = None):
        """One batch of the training loop (training.py:137-172) on `graph` (device batch): forward, losses, backward
        and — every `iters_to_accumulate`-th call — the Adam update and the LR-schedule step.  Returns the device
        tensor [pitch, dur, structure, kld] of this batch's loss values (float64, no host sync)."""
        vae = self.vae
        self._not_in_ema_weights("train_step")
        if not vae.training:
            raise RuntimeError("train_step needs vae.train()")
        if vae.flat_params.data_ptr() != self._flat_ptr:
            raise RuntimeError("the model's flat parameter buffer moved after the trainer was built; rebuild it")
        if self._guard:
            self._warn_skips()
        if self.train_metrics and self._mrows >= self._mhist.shape[0]:
            raise RuntimeError(f"the training-accuracy history is full ({self._mhist.shape[0]} unread batches): call "
                               "read_train_accuracies() first, or build the trainer with a larger metrics_capacity")
        clip = self.max_grad_norm is not None
        if clip and self._nrows >= self._nhist.shape[0]:
            raise RuntimeError(f"the gradient-norm history is full ({self._nhist.shape[0]} unread updates): call "
                               "read_grad_norms() first, or build the trainer with a larger grad_norm_capacity")
        self.grads.zero_()
        k = self.iters_to_accumulate
        self.buckets.hold = k > 1                      # micro-batches of an accumulation are not all-reduced one by one
        out = (self._native_forward_backward if self.native else self._python_forward_backward)(graph, eps)
        if self.train_metrics:
            self._mrows += 1                               # (the forward ran: a batch whose update is skipped is recorded too)
        self.micro_batches += 1
        grads = self.grads
        if k > 1:
            # training.py:149: backward of tot_loss / k, summed into .grad; the update waits for the k-th batch (:158)
            ops.grad_accumulate(self.grads, self.grad_accum, 1.0 / k, self.micro_batches % k == 1)
            if self.micro_batches % k != 0:
                return out
            self._accum_bucket.launch(0)
            mean_scale = self._accum_bucket.wait()
            grads = self.grad_accum
        else:
            mean_scale = self.buckets.wait()
        self._optimizer_update(grads, mean_scale)
        if self.sched is not None:
            self.lr = self.sched.step()
        return out

    # ---- evaluation (training.py:250-296 `evaluate`, :298-347 `_losses`, :349-497 `_accuracies`) --------------
    def evaluate_batch(self, graph, eps: Optional[torch.Tensor] = None, ema: bool = False):
        """One batch of `PolyphemusTrainer.evaluate`: eval-mode forward, the 7 losses and the 9 accuracies of the
        reference (same keys), computed by the loss / metric kernels with ONE host sync at the end (the reference
        takes 16).  Quirk kept (SURVEY B-1): the structure terms are evaluated on the target itself unless the
        trainer was built with `structure_loss_on_logits=True`.  `ema=True`: on the averaged parameters
        (`ema_weights()`; needs `ema_decay`)."""
        if ema:
            with self.ema_weights():
                return self.evaluate_batch(graph, eps)
        vae = self.vae
        was_training = vae.training
        vae.eval()
        try:
            with torch.no_grad():
                mu, lv = vae.encoder(graph)
                e = eps if eps is not None else torch.randn_like(mu)
                z = ops.reparam_fwd(mu.contiguous(), lv.contiguous(), e)
                s_logits, c_logits = vae.decoder(z, graph)
                plan = prepare_graph(graph, vae.cfg["n_bars"])
                s_t = graph.s_tensor.float().contiguous()
                out = torch.zeros(4, dtype=torch.float64, device=mu.device)
                ops.content_ce(c_logits.contiguous(), plan, want_grad=False, out=out)
                ops.kld(mu.contiguous(), lv.contiguous(), out, beta=self.beta)
                s_in = s_logits.reshape(-1).contiguous() if self.fix_structure_loss else s_t.reshape(-1)
                ops.bce_logits(s_in, s_t.reshape(-1), out, 1.0, want_grad=False)
                cc = ops.content_accuracy(c_logits.contiguous(), plan.tokens, plan.is_drum)
                sc = ops.structure_metrics(s_in, s_t.reshape(-1))
                host = torch.cat([out, cc.double(), sc.double()]).tolist()          # the one sync
        finally:
            vae.train(was_training)
        p, d, s, k = host[:4]
        losses = {"tot": p + d + s + self.beta * k, "pitch": p, "dur": d, "structure": s, "reconstruction": p + d + s,
                  "kld": k, "beta*kld": self.beta * k}
        accs = ops.accuracies_from_counts(host[4:16] + [s_t.numel(), 0, 0, 0])
        return losses, accs

    def evaluate(self, loader, ema: bool = False):
        """`PolyphemusTrainer.evaluate(loader)` (training.py:250-296): per-batch losses / accuracies averaged over the
        batches of `loader` (plain means of the per-batch values, like the reference's `mean(l)`); restores the
        training mode it found.  `ema=True`: on the averaged parameters (one swap around the whole loader)."""
        if ema:
            with self.ema_weights():
                return self.evaluate(loader)
        losses: Dict[str, list] = {}
        accs: Dict[str, list] = {}
        for graph in loader:
            lb, ab = self.evaluate_batch(graph)
            for k, v in lb.items():
                losses.setdefault(k, []).append(v)
            for k, v in ab.items():
                accs.setdefault(k, []).append(v)
        mean = lambda l: sum(l) / len(l)
        return {k: mean(l) for k, l in losses.items()}, {k: mean(l) for k, l in accs.items()}

    # ---- the parameter average ----------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if self._ema_w is None:
            raise RuntimeError(f"{what} needs HipTrainer(..., ema_decay=...)")

    def _not_in_ema_weights(self, what: str) -> None:
        if getattr(self, "_ema_swapped", False):
            raise RuntimeError(f"{what} inside `ema_weights()`: the model holds the averaged parameters there")

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside this context the model IS the averaged model: `vae.flat_params` and `self.ema` exchange their contents
        in place (`pm_buffer_swap`: no buffer moves, every parameter view and the native step's layout stay valid) and
        exchange them back on the way out, an exception included.  `evaluate`, `generate_music`, `vae.state_dict()` and
        `vae(graph)` in eval mode then read the average.  Parameters only: BatchNorm's running statistics are the live
        model's (the `AveragedModel(use_buffers=False)` convention).  Not re-entrant; `train_step`, `save_checkpoint`
        and `load_checkpoint` raise inside it."""
        self._need_ema("ema_weights()")
        self._not_in_ema_weights("ema_weights()")
        flat = self.vae.flat_params
        if flat.data_ptr() != self._flat_ptr:
            raise RuntimeError("the model's flat parameter buffer moved after the trainer was built; rebuild it")
        ops.buffer_swap(flat, self.ema)
        self._ema_swapped = True
        try:
            yield self.vae
        finally:
            ops.buffer_swap(flat, self.ema)
            self._ema_swapped = False

    def ema_state_dict(self) -> dict:
        """The averaged model in the layout of `vae.state_dict()` (the reference's keys, 255 at 8 layers; CPU copies):
        parameters from `self.ema`, buffers — BatchNorm's running statistics among them — from the live model.  Swaps
        nothing."""
        self._need_ema("ema_state_dict()")
        self._not_in_ema_weights("ema_state_dict()")
        vae = self.vae
        canon = {id(p): n for n, p in vae.named_parameters()}
        at = {k: vae._offsets[canon[id(p)]] for k, p in vae.named_parameters(remove_duplicate=False)}
        ema = self.ema.cpu()
        out = {}
        for k, v in vae.state_dict().items():
            out[k] = ema[at[k]:at[k] + v.numel()].view(v.shape).clone() if k in at else v.detach().cpu().clone()
        return out

    # ---- checkpoint interop (training.py:503-519 saves `optimizer.state_dict()` of torch.optim.Adam) ----------
    def optimizer_state_dict(self) -> dict:
        """The fused Adam's state in `torch.optim.Adam.state_dict()` layout: parameter ids follow
        `named_parameters()` order, `exp_avg` / `exp_avg_sq` are per-parameter copies of the flat
        moment buffers; loadable by `torch.optim.Adam(vae.parameters(), ...).load_state_dict`."""
        vae = self.vae
        P = dict(vae.named_parameters())
        state = {}
        t = float(self.step_count)                      # (overflow="skip": the device count, read once)
        for i, n in enumerate(vae._param_names):
            o, k = vae._offsets[n], P[n].numel()
            state[i] = {"step": torch.tensor(t),
                        "exp_avg": self.exp_avg[o:o + k].view(P[n].shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + k].view(P[n].shape).clone()}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(vae._param_names)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        """Inverse of `optimizer_state_dict`; also accepts a checkpoint written by the reference's
        `torch.optim.Adam` (parameters that never received a gradient have no entry there: their moments stay 0)."""
        vae = self.vae
        P = dict(vae.named_parameters())
        group = sd["param_groups"][0]
        if len(group["params"]) != len(vae._param_names):
            raise ValueError("optimizer state does not match the model's parameter list")
        self.lr, self.betas, self.eps = float(group["lr"]), tuple(group["betas"]), float(group["eps"])
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = set()
        for i, n in enumerate(vae._param_names):
            st = sd["state"].get(group["params"][i])
            if st is None:
                continue
            o, k = vae._offsets[n], P[n].numel()
            self.exp_avg[o:o + k].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + k].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused Adam keeps one step count")
        self.step_count = steps.pop() if steps else 0

    def save_checkpoint(self, path: str, **extra) -> None:
        """The reference's checkpoint file (`_save_model`, training.py:498-519): a `torch.save`d dict with
        'model_state_dict' (the 255 reference keys), 'optimizer_state_dict' (torch.optim.Adam layout) and
        'tot_batches'; `extra` carries the bookkeeping entries of the reference's loop (epoch, lrs, ...).  With
        `ema_decay` also 'ema_model_state_dict' (the average in the same keys) and 'ema' = {decay, n_averaged}.
        `generate.load_model` of the reference reads 'model_state_dict' from it."""
        self._not_in_ema_weights("save_checkpoint")
        ckpt = dict(extra)
        ckpt.update(tot_batches=self.micro_batches, dropout_stream={"seed": self.vae.seed, "step": self.vae._step},
                    model_state_dict={k: v.detach().cpu().clone() for k, v in self.vae.state_dict().items()},
                    optimizer_state_dict=self.optimizer_state_dict())
        if self._ema_w is not None:
            # the average beside the live model, readable by key like 'model_state_dict'; n_averaged = the applied updates
            # since it started, from the t the optimizer state just read
            t = int(float(next(iter(ckpt["optimizer_state_dict"]["state"].values()))["step"]))
            ckpt.update(ema_model_state_dict=self.ema_state_dict(),
                        ema={"decay": self.ema_decay, "n_averaged": t - self._ema_t0})
        torch.save(ckpt, path)

    def load_checkpoint(self, path: str) -> dict:
        """Restore model, Adam moments, step count and LR-schedule position from `save_checkpoint` / a reference
        checkpoint; returns the remaining entries.  With `ema_decay` the average is restored too; a file without one
        starts it from the loaded parameters.  Without `ema_decay` a file's average stays in the returned entries."""
        self._not_in_ema_weights("load_checkpoint")
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.vae.load_state_dict(ckpt.pop("model_state_dict"))
        self.load_optimizer_state_dict(ckpt.pop("optimizer_state_dict"))
        if self._ema_w is not None:
            self._load_ema(ckpt.pop("ema_model_state_dict", None), ckpt.pop("ema", None))
        self.micro_batches = int(ckpt.get("tot_batches", self.step_count * self.iters_to_accumulate))
        ds = ckpt.pop("dropout_stream", None)           # position of the counter-based dropout stream: a resumed run
        if ds is not None:                              # continues with fresh masks instead of replaying the old ones
            self.vae.seed, self.vae._step = int(ds["seed"]), int(ds["step"])
        if self.sched is not None:
            # (overflow="skip": the schedule also stepped on skipped updates, so its position is the number of update
            #  attempts, not t)
            self.sched.update_steps = self.micro_batches // self.iters_to_accumulate if self._guard else self.step_count
        return ckpt

    def _load_ema(self, sd: Optional[dict], meta: Optional[dict]) -> None:
        """The average of a checkpoint into `self.ema`; without one the average starts from the loaded parameters."""
        vae = self.vae
        if sd is None:
            self.ema.copy_(vae.flat_params.detach())
            self._ema_t0 = self.step_count
            return
        P = dict(vae.named_parameters())
        for n in vae._param_names:
            o = vae._offsets[n]
            self.ema[o:o + P[n].numel()].copy_(sd[n].reshape(-1))
        self._ema_t0 = self.step_count - int((meta or {}).get("n_averaged", self.step_count))

    def losses_dict(self, out: torch.Tensor) -> dict:
        """Host copy of the loss vector in the reference's dict layout (this DOES sync)."""
        p, d, s, k = out.tolist()
        rec = p + d + s
        return {"tot": rec + self.beta * k, "pitch": p, "dur": d, "structure": s, "reconstruction": rec, "kld": k,
                "beta*kld": self.beta * k}
