"""The guarded step across ranks (include/polyphemus_hip.h, "guarded optimizer step"): a saturation on ONE rank becomes +inf in
bucket 0 of that rank's gradient, the all-reduce carries it to every rank, and every rank skips the same update — with no
collective of its own and no host read.  Two ranks share one GPU over gloo as in test_zz_dp_gpu.py (RCCL with one device
per rank where the box has two)."""
import pytest
import torch

from util import run_ranks_sharing_one_gpu

pytestmark = pytest.mark.gpu
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)
SAT_W = "encoder.c_encoder.graph_encoder.layers.0.weight"


def _worker(rank, world, backend):
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd import _lib
        from polyphemus_amd.model import VAE
        from polyphemus_amd.synthetic import synthetic_batch
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100 + rank)                   # different initial weights: the trainer broadcasts rank 0's
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3, overflow="skip")
        assert tr.world == world
        if rank == 1:                                   # only rank 1 saturates (weight planes split at 2^4: 5000 * 16 > 65504)
            with torch.no_grad():
                dict(vae.named_parameters())[SAT_W].view(-1)[3] = 5000.0
        p0 = vae.flat_params.detach().clone()
        c0 = _lib.h2_clamp_events()
        batch = synthetic_batch(12, 2, p=0.25, seed=60 + rank).to(dev)
        eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(70 + rank)).to(dev)
        tr.train_step(batch, eps)
        torch.cuda.synchronize()
        clamps = _lib.h2_clamp_events() - c0
        return dict(before=p0.cpu().numpy(), after=vae.flat_params.detach().cpu().numpy(), clamps=clamps,
                    t=tr.step_count, skipped=int(tr.skipped_steps), stats=tr.overflow_stats(),
                    exp_avg_zero=bool((tr.exp_avg == 0).all()))
    finally:
        dist.destroy_process_group()


def test_saturation_on_one_rank_skips_the_step_on_every_rank():
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    r0, r1 = run_ranks_sharing_one_gpu(_worker, 2, (backend,), timeout=120.0)
    assert r0["clamps"] == 0 and r1["clamps"] > 0, (r0["clamps"], r1["clamps"])
    for r in (r0, r1):
        assert (r["t"], r["skipped"]) == (0, 1) and r["exp_avg_zero"]
        assert (r["before"] == r["after"]).all(), "a rank applied the update"
    assert r0["stats"] == {"skipped": 1, "non_finite": 1, "saturated": 0}        # rank 0 saw the inf of rank 1
    assert r1["stats"] == {"skipped": 1, "non_finite": 0, "saturated": 1}
    # rank 1's copy differs by its saturating weight only; both hold rank 0's broadcast otherwise
    diff = (r0["after"] != r1["after"]).nonzero()[0]
    assert diff.size == 1
