"""Data-parallel step on the GPU with two processes.  With >= 2 visible GPUs the ranks use backend "nccl" (RCCL), one
device each; on a one-GPU box they share the device over gloo (RCCL refuses two ranks on one device; the bucket / overlap
logic of `parallel.GradBuckets` is the same).  After the bucketed all-reduce + fused Adam both ranks hold identical
parameters, and they equal a single-process step fed the mean of the two ranks' gradients.

The file sorts last and its ranks are daemon children under `util.run_ranks` (hard wall-clock cap, traceback of a hung
rank, always killed): a multi-process problem can never again hide the parity tests (round-1 verdict)."""
import pytest
import torch

from util import RanksHung, run_ranks, run_ranks_sharing_one_gpu

pytestmark = pytest.mark.gpu
CFG = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=64, n_bars=2, resolution=8)


def _rank_batch(rank):
    from polyphemus_amd.synthetic import synthetic_batch
    return synthetic_batch(6, 2, p=0.25, seed=40 + rank)


def _worker(rank, world, backend):
    import datetime
    import torch.distributed as dist
    ndev = torch.cuda.device_count()
    dev = torch.device("cuda", rank % ndev)
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.model import VAE
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100 + rank)                 # different initial weights: the trainer must broadcast rank 0's
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3)
        assert tr.world == world
        eps = torch.randn(6, CFG["d"], generator=torch.Generator().manual_seed(7 + rank)).to(dev)
        tr.train_step(_rank_batch(rank).to(dev), eps)
        torch.cuda.synchronize()
        return vae.flat_params.detach().cpu().numpy(), tr.grads.detach().cpu().numpy()      # by value
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("side_delay_us", [0, 3000])
def test_two_rank_step_matches_mean_gradient_step(side_delay_us):
    """side_delay_us = 3000: every branch of the library's second stream (structure chains, weight preparation, the
    weight gradients of the decoder head and of the chord encoder) starts 3 ms late in both ranks (PM_SIDE_DELAY_US), so
    the gradients it produces are certainly NOT there when the caller's stream reaches the exchange unless that stream
    waits for the branch: the native step's join-before-bucket order (pm_vae_step_join_decoder_grads before bucket 2, the
    joins at the end of pm_vae_step_backward_encoder / _tail before buckets 1 and 0) is what makes the result right."""
    import os
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    os.environ["PM_SIDE_DELAY_US"] = str(side_delay_us)          # read by the ranks' library at load
    try:
        res = run_ranks_sharing_one_gpu(_worker, 2, (backend,), timeout=120.0)   # a rank that hangs or dies FAILS the test (RanksHung)
    finally:
        os.environ.pop("PM_SIDE_DELAY_US", None)
    (p0, g0), (p1, g1) = [(torch.from_numpy(a), torch.from_numpy(b)) for a, b in res]
    assert torch.equal(p0, p1), "ranks diverged"
    assert torch.equal(g0, g1), "all-reduced gradient differs between ranks"
    # single-process reference: same initial weights (rank 0's), gradient = mean of the two local gradients
    from polyphemus_amd import ops
    from polyphemus_amd.model import VAE
    from polyphemus_amd.trainer import HipTrainer
    grads = []
    for rank in range(2):
        torch.manual_seed(100)
        vae = VAE(**CFG, device="cuda").to("cuda")
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3)
        init = vae.flat_params.detach().clone()
        eps = torch.randn(6, CFG["d"], generator=torch.Generator().manual_seed(7 + rank)).cuda()
        vae._step = 0
        tr.train_step(_rank_batch(rank).to("cuda"), eps)
        grads.append(tr.grads.detach().clone())
    gsum = grads[0] + grads[1]
    # (the two runs add their float atomics — split-K slices, embedding sums — in different orders: 1-2e-5 of the largest
    #  element has been observed; a wrong or missing reduction is an O(1) error)
    assert float((gsum.cpu() - g0).abs().max()) <= 5e-5 * float(g0.abs().max())
    p = init.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ops.adam_step(p, gsum, m, v, 1e-3, 0.9, 0.98, 1e-9, 1, grad_scale=0.5)
    # noise-driven elements may differ by the full Adam step (2 * lr); everything else must agree tightly
    diff = (p.cpu() - p0).abs()
    assert float(diff.max()) <= 2.5e-3 and float((diff > 1e-5).float().mean()) < 0.02


def test_native_rccl_allreduce_single_rank():
    """`pm_comm_*` / `pm_allreduce` (the C-ABI exchange, csrc/comm.hip) on a one-rank communicator: RCCL loads, the
    communicator binds to this GPU, the collective runs on the caller's stream after the producing kernel."""
    from polyphemus_amd.parallel import NativeComm
    comm = NativeComm.single()
    x = torch.arange(1 << 20, dtype=torch.float32, device="cuda")
    y = x * 2.0                                        # producer on the current stream
    comm.all_reduce(y)
    torch.cuda.synchronize()
    assert torch.equal(y, x * 2.0)
    comm.close()


def _native_worker(rank, world):
    import datetime
    import torch.distributed as dist
    from polyphemus_amd.parallel import NativeComm
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        comm = NativeComm.from_torch_group()
        t = torch.full((4096,), float(rank + 1), device="cuda")
        comm.all_reduce(t)
        torch.cuda.synchronize()
        comm.close()
        return float(t[0]), float(t[-1])
    finally:
        dist.destroy_process_group()


def test_native_rccl_allreduce_two_gpus():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    assert run_ranks(_native_worker, 2, timeout=120.0) == [(3.0, 3.0), (3.0, 3.0)]


def _gtm_batch(rank):
    from polyphemus_amd.synthetic import synthetic_batch
    return synthetic_batch(4 + 4 * rank, 2, p=0.25, seed=60 + rank)      # 4 and 8 samples: different token counts


def _gtm_worker(rank, world, backend, d=64):
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.model import VAE
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100)
        vae = VAE(**{**CFG, "d": d}, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3, global_token_mean=True)
        b = _gtm_batch(rank)
        eps = torch.randn(b.s_tensor.shape[0] // 2, d, generator=torch.Generator().manual_seed(7 + rank)).to(dev)
        tr.train_step(b.to(dev), eps)
        torch.cuda.synchronize()
        return tr.grads.detach().cpu().numpy()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("d", [64, 128])
def test_global_token_mean_weights_the_ranks_by_their_token_counts(d):
    """CE `ignore_index` means (training.py:316-323) under data parallelism: with `global_token_mean` the summed
    gradient equals sum_r (n_r * world / n_total) * g_r, g_r = the rank's own local-mean gradient — i.e. its mean over the
    ranks is the gradient of the token mean over the global batch (per-replica BatchNorm statistics apart).  d = 128: d/2 = 64
    is a width of the weight-plane kernel of the fused head (k_unembed_ce_planes), which then receives `ce_scale` in a real
    two-rank run; at d = 64 the head takes the fp32-MFMA kernel."""
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    cfg = {**CFG, "d": d}
    res = run_ranks_sharing_one_gpu(_gtm_worker, 2, (backend, d), timeout=120.0)      # a rank that hangs or dies FAILS the test (RanksHung)
    got = torch.from_numpy(res[0])
    assert torch.equal(got, torch.from_numpy(res[1]))
    from polyphemus_amd.model import VAE
    from polyphemus_amd.trainer import HipTrainer
    grads, counts = [], []
    for rank in range(2):
        torch.manual_seed(100)
        vae = VAE(**cfg, device="cuda").to("cuda")
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3)
        b = _gtm_batch(rank)
        eps = torch.randn(b.s_tensor.shape[0] // 2, d, generator=torch.Generator().manual_seed(7 + rank)).cuda()
        tr.train_step(b.to("cuda"), eps)
        grads.append(tr.grads.detach().cpu().double())
        counts.append(float((b.tokens[:, 1:, 0] != 130).sum()))
    assert counts[0] != counts[1]
    want = sum(g * (n * 2.0 / sum(counts)) for g, n in zip(grads, counts))
    assert float((got.double() - want).abs().max()) <= 2e-5 * float(want.abs().max())


def _nccl1_worker(rank, world):
    """One rank, backend nccl (RCCL), exchange path forced on: the three gradient buckets really travel through
    ncclAllReduce on RCCL's stream while the backward continues on the compute stream."""
    import datetime
    import os
    import torch.distributed as dist
    os.environ["PM_DP_FORCE"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.model import VAE
        from polyphemus_amd.synthetic import synthetic_batch
        from polyphemus_amd.trainer import HipTrainer
        cfg = dict(dropout=0, batch_norm=True, gnn_n_layers=4, d=128, n_bars=2, resolution=8)
        batch = synthetic_batch(64, 2, p=0.25, seed=5).to("cuda")
        eps = torch.randn(64, 128, generator=torch.Generator().manual_seed(1)).cuda()
        out = []
        for force in (True, False):
            torch.manual_seed(0)
            vae = VAE(**cfg, device="cuda").to("cuda")
            vae.train()
            vae.msg_dropout = 0.0
            tr = HipTrainer(vae, lr=1e-3)
            assert tr.buckets.active
            tr.buckets.disabled = not force
            g1 = None
            for i in range(3):
                tr.train_step(batch, eps)
                if i == 0:
                    g1 = tr.grads.detach().cpu().numpy()      # same weights in both runs: comparable to rounding noise
            torch.cuda.synchronize()
            out.append((vae.flat_params.detach().cpu().numpy(), g1))
        return out
    finally:
        dist.destroy_process_group()


def test_bucketed_exchange_over_rccl_single_rank():
    """RCCL has never run with more than one rank on the builder's one-GPU boxes; this at least runs the real
    `ncclAllReduce` launches of the trainer (three async buckets overlapping the backward, then the fused Adam) on
    backend "nccl" and checks that the result equals the same steps without the exchange: a stream-ordering bug
    (all-reduce reading a bucket before its producers finished, Adam reading it before the all-reduce) would show."""
    (p_dp, g_dp), (p_ref, g_ref) = run_ranks(_nccl1_worker, 1, timeout=150.0)[0]
    gd, gr = torch.from_numpy(g_dp), torch.from_numpy(g_ref)
    assert float((gd - gr).abs().max()) <= 2e-4 * float(gr.abs().max())        # (atomics-order noise between two runs)
    assert float((torch.from_numpy(p_dp) - torch.from_numpy(p_ref)).abs().max()) <= 6.5e-3   # 3 Adam steps at lr 1e-3
    assert float((torch.from_numpy(p_dp) - torch.from_numpy(p_ref)).abs().mean()) < 2e-4      # (Adam at lr 1e-3 amplifies rounding noise)


def _sync_samples():
    """12 synthetic two-bar samples (one generator), as sample dicts: ranks take [0:6] and [6:12], the single device all."""
    import numpy as np
    from polyphemus_amd.synthetic import disk_sample, sample_from_disk
    rng = np.random.default_rng(77)
    return [sample_from_disk(*disk_sample(rng, 2, 0.25), 2) for _ in range(12)]


def _sync_worker(rank, world, backend):
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    try:
        from polyphemus_amd.graphs import collate_samples
        from polyphemus_amd.model import VAE
        from polyphemus_amd.trainer import HipTrainer
        torch.manual_seed(100)
        vae = VAE(**CFG, device=dev).to(dev)
        vae.train()
        vae.msg_dropout = 0.0
        tr = HipTrainer(vae, lr=1e-3, sync_bn=True, global_token_mean=True)
        assert not tr.native and vae.engine._sync_on
        batch = collate_samples(_sync_samples()[6 * rank:6 * rank + 6], 2).to(dev)
        eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(3))[6 * rank:6 * rank + 6].to(dev)
        tr.train_step(batch, eps)
        torch.cuda.synchronize()
        return tr.grads.detach().cpu().numpy(), vae.flat_buffers.detach().cpu().numpy()
    finally:
        dist.destroy_process_group()


def test_sync_bn_data_parallel_step_equals_single_device_global_batch():
    """with synchronised BatchNorm (all ~25 norms: GCL, CNN, heads, gate, embeddings) and the global token
    mean of the CE terms, the averaged gradient of two ranks on 6 samples each equals the single-device gradient on the
    12 samples — the reference's semantics, whose BatchNorm statistics and loss means span the whole batch —, and the
    running statistics agree."""
    backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    res = run_ranks_sharing_one_gpu(_sync_worker, 2, (backend,), timeout=150.0)      # a rank that hangs or dies FAILS the test (RanksHung)
    g_dp = torch.from_numpy(res[0][0]).double() / 2.0           # the buckets hold the SUM over the ranks
    assert torch.equal(torch.from_numpy(res[0][0]), torch.from_numpy(res[1][0]))
    from polyphemus_amd.graphs import collate_samples
    from polyphemus_amd.model import VAE
    from polyphemus_amd.trainer import HipTrainer
    torch.manual_seed(100)
    vae = VAE(**CFG, device="cuda").to("cuda")
    vae.train()
    vae.msg_dropout = 0.0
    tr = HipTrainer(vae, lr=1e-3, native=False)
    eps = torch.randn(12, CFG["d"], generator=torch.Generator().manual_seed(3)).cuda()
    tr.train_step(collate_samples(_sync_samples(), 2).to("cuda"), eps)
    g_one = tr.grads.detach().cpu().double()
    gmax = float(g_one.abs().max())
    # measured 1.8e-7 / 7.8e-7 (tools/dp_equivalence.py; with per-replica statistics: 2.2e-1 / 8.0e-1)
    assert float((g_dp - g_one).abs().max()) <= 1e-5 * gmax, float((g_dp - g_one).abs().max()) / gmax
    assert float(((g_dp - g_one) ** 2).sum().sqrt() / (g_one ** 2).sum().sqrt()) < 1e-5
    b_dp, b_one = torch.from_numpy(res[0][1]).double(), vae.flat_buffers.detach().cpu().double()
    assert float((b_dp - b_one).abs().max()) <= 1e-5 * max(1.0, float(b_one.abs().max()))
