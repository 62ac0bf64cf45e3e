"""Gradient clipping across ranks (include/polyphemus_hip.h, "gradient clipping by the global norm"): the norm is taken behind
the all-reduce, on the gradient every rank holds alike, so every rank computes the same (norm, coef) bits and applies the same
update with no collective of its own.  Two ranks share one GPU over gloo as in test_zz_overflow_dp_gpu.py (RCCL with one
device per rank where the box has two)."""
import pytest
import torch

from util import run_ranks_sharing_one_gpu

pytestmark = pytest.mark.gpu
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)
MAX_NORM = 1e-2             # far below the gradient norm of this model at initialisation (asserted: coef < 1)


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
        tr = HipTrainer(vae, lr=1e-3, overflow="skip", max_grad_norm=MAX_NORM)
        assert tr.world == world
        mean_norms = []
        for k in range(2):
            batch = synthetic_batch(12, 2, p=0.25, seed=60 + 2 * k + rank).to(dev)
            eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(70 + 2 * k + rank)).to(dev)
            tr.train_step(batch, eps)
            mean_norms.append(float((tr.grads.double() / world).norm()))      # tr.grads: the sum over ranks
        rows = tr.read_grad_norms()
        return dict(rows=rows, mean_norms=mean_norms, after=vae.flat_params.detach().cpu().numpy(), t=tr.step_count,
                    skipped=int(tr.skipped_steps))
    finally:
        dist.destroy_process_group()


def test_every_rank_records_the_same_norm_and_applies_the_same_clipped_update():
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    r0, r1 = run_ranks_sharing_one_gpu(_worker, 2, (backend,), timeout=120.0)
    assert len(r0["rows"]) == 2
    # bitwise: repr of a double round-trips
    assert [tuple(map(float.hex, r)) for r in r0["rows"]] == [tuple(map(float.hex, r)) for r in r1["rows"]]
    for r in (r0, r1):
        assert (r["t"], r["skipped"]) == (2, 0)
        for (norm, coef), ref in zip(r["rows"], r["mean_norms"]):
            assert abs(norm - ref) <= 1e-9 * ref, (norm, ref)
            assert coef < 1 and coef == min(1.0, float(torch.tensor(MAX_NORM, dtype=torch.float32)) / (norm + 1e-6))
    assert (r0["after"] == r1["after"]).all(), "the ranks' parameters diverged"
