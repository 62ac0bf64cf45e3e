"""Training accuracies across ranks: each rank counts its own batch (the counts of that batch on one device), and
`read_train_accuracies(reduce=True)` sums the counts over the process group — the accuracies of the concatenated batch — on
every rank.  Two ranks share one GPU over gloo as in test_zz_overflow_dp_gpu.py."""
import math

import pytest
import torch

from util import run_ranks_sharing_one_gpu

pytestmark = pytest.mark.gpu
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=128, n_bars=2, resolution=8)


def _batch(rank):
    from polyphemus_amd.synthetic import synthetic_batch
    return synthetic_batch(12, 2, p=0.25, seed=80 + rank)


def _eps(rank):
    return torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(90 + rank))


def _worker(rank, world, backend):
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.model import VAE
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100 + rank)                   # the trainer broadcasts rank 0's weights
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=5e-6, train_metrics=True)
        assert tr.world == world
        tr.train_step(_batch(rank).to(dev), _eps(rank).to(dev))
        local = tr.last_train_counts.tolist()
        reduced = tr.read_train_accuracies(reduce=True)
        return dict(local=local, reduced=reduced)
    finally:
        dist.destroy_process_group()


def test_rank_counts_and_reduced_accuracies():
    from polyphemus_amd import ops
    from polyphemus_amd.model import VAE
    from polyphemus_amd.trainer import HipTrainer
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    r0, r1 = run_ranks_sharing_one_gpu(_worker, 2, (backend,), timeout=120.0)
    dev = torch.device("cuda", 0)
    for rank, r in enumerate((r0, r1)):                 # the same batch on one device, from rank 0's initial weights
        torch.manual_seed(100)
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=5e-6, train_metrics=True)
        tr.train_step(_batch(rank).to(dev), _eps(rank).to(dev))
        assert r["local"] == tr.last_train_counts.tolist(), rank
        assert r["local"][1] > 0
    want = ops.accuracies_from_counts([a + b for a, b in zip(r0["local"], r1["local"])])
    for r in (r0, r1):
        assert len(r["reduced"]) == 1
        got = r["reduced"][0]
        assert all((math.isnan(got[k]) and math.isnan(v)) or got[k] == v for k, v in want.items()), (got, want)
