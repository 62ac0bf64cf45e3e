"""The parameter average across ranks (include/polyphemus_hip.h, "exponential moving average of the parameters"): it starts
from the weights rank 0 broadcast and moves inside the Adam launch on the gradient every rank holds alike, so every rank
keeps the same bits with no collective of its own — here with the guarded, clipped update.  Two ranks share one GPU over gloo
as in test_zz_gradclip_dp_gpu.py (RCCL with one device per rank where the box has two)."""
import numpy as np
import pytest
import torch

from util import run_ranks_sharing_one_gpu

pytestmark = pytest.mark.gpu
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)
DECAY = 0.9
BOUND = 2.0 ** -22           # per update, of max(|ema|, |p|): tests/test_ema_gpu.py


def _worker(rank, world, backend):
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.model import VAE
        from polyphemus_amd.synthetic import synthetic_batch
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100 + rank)                   # different initial weights: the trainer broadcasts rank 0's
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        own = vae.flat_params.detach().cpu().numpy().copy()
        tr = HipTrainer(vae, lr=1e-3, overflow="skip", max_grad_norm=1e-2, ema_decay=DECAY)
        assert tr.world == world
        start = tr.ema.cpu().numpy().copy()
        params = [vae.flat_params.detach().cpu().numpy().copy()]
        for k in range(2):
            batch = synthetic_batch(12, 2, p=0.25, seed=60 + 2 * k + rank).to(dev)
            eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(70 + 2 * k + rank)).to(dev)
            tr.train_step(batch, eps)
            params.append(vae.flat_params.detach().cpu().numpy().copy())
        return dict(own=own, start=start, params=params, ema=tr.ema.cpu().numpy(), t=tr.step_count,
                    skipped=int(tr.skipped_steps))
    finally:
        dist.destroy_process_group()


def test_every_rank_keeps_the_same_average_from_rank_zeros_weights():
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    r0, r1 = run_ranks_sharing_one_gpu(_worker, 2, (backend,), timeout=120.0)
    assert not (r0["own"] == r1["own"]).all()
    for r in (r0, r1):
        assert (r["t"], r["skipped"]) == (2, 0)
        assert (r["start"] == r0["own"]).all(), "the average does not start from the weights rank 0 broadcast"
        assert (r["params"][0] == r0["own"]).all()
    assert (r0["ema"].view(np.uint32) == r1["ema"].view(np.uint32)).all(), "the ranks' averages diverged"
    assert (r0["params"][2] == r1["params"][2]).all()
    # the float64 recurrence from rank 0's broadcast weights over the parameters each update left
    w = float(np.float32(1.0 - DECAY))
    e = r0["own"].astype(np.float64)
    seen = np.abs(e)
    for p in r0["params"][1:]:
        p = p.astype(np.float64)
        e = e + w * (p - e)
        seen = np.maximum(seen, np.maximum(np.abs(p), np.abs(e)))
    excess = np.abs(r0["ema"].astype(np.float64) - e) - 2 * BOUND * seen
    assert float(excess.max()) <= 0.0, float(excess.max())
    assert not (r0["ema"] == r0["params"][2]).all()
