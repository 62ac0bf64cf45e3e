"""Shared helpers for the parity tests: golden loading and the 1e-4 relative metric."""
import json
import os

import numpy as np
import torch

from polyphemus_amd.graphs import BarGraphBatch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REL_TOL = 1e-4          # BASELINE.json north_star: "outputs matching reference within 1e-4 rel"


def rel_err(a, b):
    """max|a-b| / max|b|  (SURVEY §8(d)); 0 when both are all-zero."""
    a = torch.as_tensor(a, dtype=torch.float64).cpu()
    b = torch.as_tensor(b, dtype=torch.float64).cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    den = float(b.abs().max()) if b.numel() else 0.0
    num = float((a - b).abs().max()) if b.numel() else 0.0
    return num / den if den > 0 else num


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    cfg = json.loads(str(z["cfg"]))
    return z, cfg


def batch_from_golden(z, cfg) -> BarGraphBatch:
    """The reference-built batch of a golden case as a BarGraphBatch (CPU)."""
    from polyphemus_amd.graphs import batch_flags
    ei, et = torch.from_numpy(z["in/edge_index"].astype(np.int64)), torch.from_numpy(z["in/etype"].astype(np.int32))
    n_slots, unique = batch_flags(torch.from_numpy(z["in/tokens"].astype(np.int32)), ei, et, int(z["in/num_nodes"]))
    return BarGraphBatch(
        n_slots=n_slots, track_unique=unique,        # what `collate_samples` attaches: selects the measured native path
        edge_index=torch.from_numpy(z["in/edge_index"].astype(np.int64)),
        edge_type=torch.from_numpy(z["in/etype"].astype(np.int32)),
        edge_dist=torch.from_numpy(z["in/edist"].astype(np.int32)),
        tokens=torch.from_numpy(z["in/tokens"].astype(np.int32)),
        s_tensor=torch.from_numpy(z["in/s_tensor"].astype(np.float32)),
        is_drum=torch.from_numpy(z["in/is_drum"].astype(bool)),
        bars=torch.from_numpy(z["in/bars"].astype(np.int64)),
        batch=torch.from_numpy(z["in/batch"].astype(np.int64)),
        num_nodes=int(z["in/num_nodes"]), n_bars=cfg["n_bars"])


def state_dict_from_golden(z, prefix="sd/"):
    if prefix == "sd/" and "sd_sha256" in z.files:
        # slim fixture: the initial state is the reference's default init under torch.manual_seed(0); the product's
        # module tree reproduces it bit for bit, which the stored digest of the reference's tensors proves here
        import hashlib
        from polyphemus_amd.model import VAE
        torch.manual_seed(0)
        sd = {k: v.detach().clone() for k, v in VAE(**json.loads(str(z["cfg"])), device=torch.device("cpu")).state_dict().items()}
        h = hashlib.sha256()
        for k, v in sd.items():
            h.update(k.encode()); h.update(v.numpy().tobytes())
        assert h.hexdigest() == str(z["sd_sha256"]), "default init differs from the reference's (fixture digest)"
        return sd
    return {k[len(prefix):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(prefix)}


# ---- counter-based dropout stream of the HIP path, restated in numpy (csrc/common.h) ----
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = x.astype(np.uint64) & _M32
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def dropout_keep_np(seed, layer_uid, eids, d, p):
    """keep[e, c] of pm_dropout_keep(seed, layer, eid, channel) for p in [0,1): float32 0/1."""
    eids = np.asarray(eids, dtype=np.uint64)
    k0 = _mix32(np.array([(seed & 0xFFFFFFFF) ^ (((layer_uid + 1) * 0x9E3779B9) & 0xFFFFFFFF)], np.uint64))[0]
    ek = _mix32(k0 ^ ((eids * np.uint64(0x85EBCA6B) + np.uint64(0x27D4EB2F)) & _M32))
    grp = ((np.arange(d, dtype=np.uint64) >> np.uint64(2)) * np.uint64(0xC2B2AE35)) & _M32    # one mix per 4 channels,
    lane = np.array([1, 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D], np.uint64)[np.arange(d) & 3]        # times a per-lane odd constant
    h = (_mix32((ek[:, None] + grp[None, :]) & _M32) * lane[None, :]) & _M32
    thresh = np.uint64(int(np.float32(p) * np.float32(16777216.0)))
    return ((h >> np.uint64(8)) >= thresh).astype(np.float32)


def _mul32(x, k):
    """(x * k) mod 2^32 for int64 x, k in [0, 2^32) (k an int or a tensor): in two 16-bit halves of k, so that no product
    leaves int64"""
    return (x * (k & 0xFFFF) + (((x * (k >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF


def _mix32_t(x):
    x = x ^ (x >> 16); x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15); x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


_LANE = (1, 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D)


def dropout_hash_torch(seed, layer_uid, eids, d):
    """pm_dropout_hash(seed, layer, eid, channel) (the top 24 bits of the element hash, csrc/common.h) for every edge id of
    `eids` (int64, any device) and channel < d, in torch on int64 with 32-bit masking: [len(eids), d] int64."""
    eids = torch.as_tensor(eids, dtype=torch.int64)
    dev = eids.device
    k0 = _mix32_t(torch.tensor([(seed & 0xFFFFFFFF) ^ (((layer_uid + 1) * 0x9E3779B9) & 0xFFFFFFFF)], dtype=torch.int64, device=dev))
    ek = _mix32_t(k0 ^ ((_mul32(eids & 0xFFFFFFFF, 0x85EBCA6B) + 0x27D4EB2F) & 0xFFFFFFFF))
    ch = torch.arange(d, dtype=torch.int64, device=dev)
    grp = _mul32(ch >> 2, 0xC2B2AE35)                                               # one mix per 4 channels,
    lane = torch.tensor(_LANE, dtype=torch.int64, device=dev)[ch & 3]               # times a per-lane odd constant
    return _mul32(_mix32_t((ek[:, None] + grp[None, :]) & 0xFFFFFFFF), lane[None, :]) >> 8


def dropout_keep_torch(seed, layer_uid, eids, d, p):
    """`dropout_keep_np` from `dropout_hash_torch`, on the device of `eids`: float32 0/1 [len(eids), d], bit for bit the same
    mask.  What the edge-chunked oracle evaluates per chunk, where numpy's single thread over 1e9 elements per layer would
    dominate the test."""
    thresh = int(np.float32(p) * np.float32(16777216.0))
    return (dropout_hash_torch(seed, layer_uid, eids, d) >= thresh).to(torch.float32)


def layer_uid_of(key: str) -> int:
    """GCL parameter prefix -> layer uid used by the HIP path (encoder GCN 0.., decoder GCN 1000..)."""
    base = 0 if key.startswith("encoder.") else 1000
    return base + int(key.rsplit(".", 1)[1])


# ---- multi-process harness of the data-parallel tests (CPU gloo and GPU) ----------------------------------
def _rank_main(fn, rank, world, port, q, dump_dir, hang_after, args):
    """Child entry: rendezvous on 127.0.0.1, run `fn(rank, world, *args)`, ship its result or its traceback."""
    import faulthandler
    import traceback
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), GLOO_SOCKET_IFNAME=os.environ.get("GLOO_SOCKET_IFNAME", "lo"))
    dump = open(os.path.join(dump_dir, f"rank{rank}.trace"), "w")
    faulthandler.enable(dump)
    faulthandler.dump_traceback_later(hang_after, exit=True, file=dump)     # a hung rank names its frame and dies
    try:
        q.put((rank, "ok", fn(rank, world, *args)))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
    finally:
        faulthandler.cancel_dump_traceback_later()


class RanksHung(RuntimeError):
    pass


def _share_probe(rank, world):
    """two processes on ONE device: each opens it, runs a kernel and meets the other in a gloo all-reduce"""
    import datetime
    import torch.distributed as dist
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=30))
    try:
        t = torch.ones(1024, device=dev) * (rank + 1)
        torch.cuda.synchronize()
        c = t.cpu()
        dist.all_reduce(c)
        return float(c[0])
    finally:
        dist.destroy_process_group()


_SHARE_OK = {}            # world -> did the probe pass on this box (decided once per session, BEFORE the first test runs)


def run_ranks_sharing_one_gpu(fn, world, args=(), timeout=90.0):
    """`run_ranks` for the data-parallel tests.  With as many devices as ranks a rank that hangs or dies FAILS the test.  On a
    one-GPU box the ranks share the device over gloo: a minimal probe (two processes open the device side by side and meet in
    an all-reduce) runs FIRST, once per session; if it fails — an environment property of the box — the test is skipped up front
    with that reason.  Once the probe has passed, any hang or death of a rank is the code's and fails the test (a
    deadlock of the step must not be reported as a skip on exactly the boxes the suite runs on)."""
    if torch.cuda.device_count() < world:
        if world not in _SHARE_OK:
            try:
                _SHARE_OK[world] = run_ranks(_share_probe, world, (), timeout=60.0) == [float(world * (world + 1) // 2)] * world
            except (RanksHung, AssertionError):
                _SHARE_OK[world] = False
        if not _SHARE_OK[world]:
            import pytest
            pytest.skip(f"{world} processes cannot share this box's single GPU (the up-front probe failed): environmental, "
                        f"not a parity failure")
    return run_ranks(fn, world, args, timeout)


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_ranks(fn, world, args=(), timeout=90.0):
    """Run `fn(rank, world, *args)` in `world` fresh spawn processes (daemon, never re-exec'd) and return their results
    in rank order.  A rank that raises fails the caller with the rank's traceback; ranks that do not answer within
    `timeout` seconds are killed and RanksHung carries their faulthandler dumps.  Children never outlive the call."""
    import tempfile
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    dump_dir = tempfile.mkdtemp(prefix="pm_ranks_")
    procs = [ctx.Process(target=_rank_main, args=(fn, r, world, port, q, dump_dir, max(timeout - 10.0, 5.0), args),
                         daemon=True) for r in range(world)]
    res = {}
    try:
        for p in procs:
            p.start()
        deadline = time.time() + timeout
        while len(res) < world and time.time() < deadline:
            try:
                rank, status, payload = q.get(timeout=1.0)
            except Exception:
                if any(p.exitcode not in (None, 0) for p in procs) and q.empty():
                    time.sleep(0.5)
                    if q.empty():
                        break
                continue
            if status == "error":
                raise AssertionError(f"rank {rank} raised:\n{payload}")
            res[rank] = payload
        if len(res) < world:
            traces = []
            for r in range(world):
                try:
                    traces.append(f"--- rank {r} (exit code {procs[r].exitcode}) ---\n" +
                                  open(os.path.join(dump_dir, f"rank{r}.trace")).read()[-3000:])
                except OSError:
                    pass
            raise RanksHung(f"{world - len(res)} of {world} ranks gave no result within {timeout:.0f} s\n" + "\n".join(traces))
        for p in procs:
            p.join(timeout=20)
        bad = [(r, p.exitcode) for r, p in enumerate(procs) if p.exitcode not in (0, None)]
        assert not bad, f"ranks exited non-zero: {bad}"
        return [res[r] for r in range(world)]
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=5)
            if p.is_alive():
                p.kill()
                p.join(timeout=5)


def fp64_oracle_grads(z, cfg):
    """Gradients of the reference training step of a golden case, computed by oracle/vae_cpu.py in fp64 (one thread):
    the anchor of the gradient tolerances (the golden's own fp32 gradients sit up to 2.7e-2 of a tensor's scale from
    exact arithmetic; tools/golden_fp64_diag.py)."""
    from oracle import vae_cpu
    names = [str(n) for n in z["param_names"]]
    sd0 = state_dict_from_golden(z)
    P, _ = vae_cpu.split_state({k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd0.items()}, names)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _, _, g = vae_cpu.train_step(_as_dtype(batch_from_golden(z, cfg), torch.float64), P, names, cfg,
                                     torch.optim.SGD([P[k] for k in names], lr=0.0),
                                     torch.from_numpy(z["in/eps"]).double(), msg_dropout=0.0)
    finally:
        torch.set_num_threads(n)
    return g


# ---- full-size parity: the native HIP step against the CPU oracle in fp32 AND fp64 ------------------------------
FULLSIZE = {
    # BASELINE.json configs[1..2] and one GPU's shard of configs[4]; message dropout replayed where the mask is cheap
    "configs1_lmd2_b256_d256": dict(B=256, nb=2, d=256, L=8, p=0.25, dense=False, msg_p=0.1, seed=1234),
    "configs2_lmd16_b64_d256": dict(B=64, nb=16, d=256, L=8, p=0.25, dense=False, msg_p=0.1, seed=1234),
    "configs4_dense_shard_b8_d512": dict(B=8, nb=2, d=512, L=8, p=1.0, dense=True, msg_p=0.0, seed=1234),
    # the reference's own training configuration (training.json:2-9: batch 256, d = 512, 8 layers, 2 bars)
    "training_json_b256_d512": dict(B=256, nb=2, d=512, L=8, p=0.25, dense=False, msg_p=0.1, seed=1234),
    # configs[1] with the batch of seed 1235: 258 row tiles for 256 CUs — two tiles of every GCL launch and one of every
    # chord product run as 32-row halves (csrc/tile_order.h); rank 1's batch of a multi-GPU bench run
    "configs1_seed1235_258_tiles": dict(B=256, nb=2, d=256, L=8, p=0.25, dense=False, msg_p=0.1, seed=1235),
}
# a small d = 128 step (the kernels of gcl.hip at their narrowest width) for the forced-decision test: ADVICE r5 — at small sizes the
# fused-vs-unfused comparison only bounds the whole gradient by what a few flipped ReLU decisions can move it
SMALLSIZE = {
    "small_b24_d128_l3": dict(B=24, nb=2, d=128, L=3, p=0.25, dense=False, msg_p=0.1, seed=31),
}
# configs[4]'s dense shard at B = 8 with message dropout on: the dense route's dropout stream against the oracle under the
# step's ReLU decisions (test_gradient_is_the_fp64_oracles_under_the_relu_decisions_the_step_took only: no GRAD_CAPS entry)
FORCED_ONLY = {
    "configs4_dense_shard_b8_d512_msg_p01": dict(B=8, nb=2, d=512, L=8, p=1.0, dense=True, msg_p=0.1, seed=1234),
}
# one GPU's shard of configs[4] at its real size (B = 64: N = 16,384 nodes, 2.08 M edges): against the fp64 oracle through
# its edge-chunked aggregation (vae_cpu.chunked_aggregation: the per-edge fp64 tensors of the default path take 8.5 GB each)
# under the step's ReLU decisions, and property checks (tests/test_fullsize_gpu.py)
DENSE_SHARD_B64 = dict(B=64, nb=2, d=512, L=8, p=1.0, dense=True, msg_p=0.1, seed=1234)


PROF_CLASSES = 40            # launch classes of pm_prof_begin / pm_prof_end (PM_PROF_NCLASS of csrc/prof.h)


def _as_dtype(batch, dtype):
    """The reference-format float inputs of a CPU batch (c_tensor, edge_attrs, s_tensor) in `dtype`."""
    out = BarGraphBatch(**{k: v for k, v in batch.__dict__.items() if not k.startswith("_")})
    out.__dict__["_c_tensor"] = batch.c_tensor.to(dtype)
    out.__dict__["_edge_attrs"] = batch.edge_attrs.to(dtype)
    out.s_tensor = batch.s_tensor.to(dtype)
    return out


def hip_fullsize_step(spec, dev="cuda", lr=5e-6, keep=None):
    """One native HIP training step (the measured variant) on the synthetic batch of `spec`, default-init weights under
    manual_seed(0) and a fixed eps: model outputs, losses, gradients, the step variant, and what the oracle needs to
    replay it (batch, state dict, eps, the two dropout seeds).  Optional keys of `spec`: `dropout` (0), `batch_norm` (True) — the
    model's constructor switches —, `track_unique` (what the batch carries; False: the 7-block aggregates), `n_slots` (the token
    slots the batch declares active), `train_metrics` (False: the trainer's accuracy counts) and `keep_logits` (True; False is the
    bench's head — the logits are not stored, `step_outputs()` is skipped and `outputs` is None)."""
    import time
    from polyphemus_amd.model import VAE
    from polyphemus_amd.synthetic import synthetic_batch
    from polyphemus_amd.trainer import HipTrainer
    cfg = dict(dropout=spec.get("dropout", 0), batch_norm=spec.get("batch_norm", True), gnn_n_layers=spec["L"], d=spec["d"],
               n_bars=spec["nb"], resolution=8)
    cpu = synthetic_batch(spec["B"], spec["nb"], p=spec["p"], seed=spec["seed"], dense=spec["dense"])
    if "track_unique" in spec:
        cpu.track_unique = bool(spec["track_unique"])
    if "n_slots" in spec:
        cpu.n_slots = int(spec["n_slots"])
    torch.manual_seed(0)
    vae = VAE(**cfg, device=dev).to(dev)
    vae.train()
    vae.msg_dropout = spec["msg_p"]
    sd = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    names = [n for n, _ in vae.named_parameters()]
    eps = torch.randn(spec["B"], spec["d"], generator=torch.Generator().manual_seed(99))
    tr = HipTrainer(vae, lr=lr, structure_loss_on_logits=bool(spec.get("fix_structure", False)),
                    train_metrics=bool(spec.get("train_metrics", False)))
    tr.keep_logits = bool(spec.get("keep_logits", True))
    step0 = vae._step
    t0 = time.time()
    # launch-class counters of the in-library profiler: WHICH kernels the step took (35 / 36 / 37 = the three GCL kernels of
    # gcl.hip / wide.hip, 38 = the chord products of linear.hip / wide.hip, 27 / 28 / 26 = the grouped planes products)
    import ctypes
    from polyphemus_amd._lib import lib
    L = lib()
    L.pm_prof_configure(-1, 1)
    L.pm_prof_begin(1024)
    gpu_batch = cpu.to(dev)
    from polyphemus_amd import _lib as _lm
    _lm.h2_clamp_events(reset=True)
    got_l = tr.losses_dict(tr.train_step(gpu_batch, eps.to(dev)))
    clamps = _lm.h2_clamp_events()
    ms, work, cnt = (ctypes.c_double * 64)(), (ctypes.c_double * 64)(), (ctypes.c_int64 * 64)()
    L.pm_prof_end(*(ctypes.cast(a, ctypes.c_void_p) for a in (ms, work, cnt)))
    if tr.keep_logits:
        (s_h, c_h), mu_h, lv_h = tr.step_outputs()
    info = tr.step_info()
    info["h2_clamp_events"] = clamps              # threads of the pair-format splits that saturated in this step (must be 0)
    info["launches"] = {"gcl_fwd": int(cnt[35]), "gcl_dagg": int(cnt[36]), "gcl_dw": int(cnt[37]), "rows_w": int(cnt[38]), "rows_tn": int(cnt[39]),
                        "planesB_nn": int(cnt[27]), "planesB_nt": int(cnt[28]), "planes_tn": int(cnt[26]),
                        "segreduce_fwd": int(cnt[33]), "segreduce_bwd": int(cnt[34])}
    info["launch_counts"] = [int(cnt[i]) for i in range(PROF_CLASSES)]     # every launch class of the profiler, in its order
    hip = dict(s_logits=s_h.cpu(), c_logits=c_h.cpu(), mu=mu_h.cpu(), log_var=lv_h.cpu()) if tr.keep_logits else None
    hip_g = {n: tr._G[n].detach().cpu() for n in names}
    t_hip = time.time() - t0
    vae._step = step0
    seeds = {"encoder": vae._next_seed(), "decoder": vae._next_seed()}
    out = dict(cfg=cfg, cpu=cpu, sd=sd, names=names, eps=eps, losses=got_l, outputs=hip, grads=hip_g, info=info,
               seconds=t_hip, seeds=seeds)
    if keep is not None:                      # the live objects, for tests that take further steps on the same model
        keep.update(vae=vae, trainer=tr, batch=gpu_batch, eps=eps.to(dev), step0=step0)
    return out


def oracle_fullsize(spec, run, dtypes=(("o64", torch.float64), ("o32", torch.float32)), chunk=None, device=None, states=None):
    """oracle/vae_cpu.py on what `hip_fullsize_step` ran (same weights, eps and — replayed from the counter hash — the
    same message-dropout mask), per dtype: (outputs, losses, gradients), and the seconds each took.  With `chunk` the GCL
    aggregations run edge-chunked on `device` (vae_cpu.chunked_aggregation) and the dropout masks are evaluated per chunk
    there (`dropout_keep_torch`, nothing cached).  With a dict `states`, states[tag] receives the buffers (running
    statistics, num_batches_tracked) the oracle's step left in its state."""
    import contextlib
    import time
    from oracle import vae_cpu
    cfg, cpu, sd, names, eps, seeds = (run[k] for k in ("cfg", "cpu", "sd", "names", "eps", "seeds"))
    masks = {}

    def keep(key, eids, dd):
        if chunk is not None:
            return dropout_keep_torch(seeds[key.split(".")[0]], layer_uid_of(key), eids, dd, spec["msg_p"])
        k = (key, dd, eids.numel(), int(eids[0]) if eids.numel() else -1, int(eids[-1]) if eids.numel() else -1)
        if k not in masks:
            masks[k] = torch.from_numpy(dropout_keep_np(seeds[key.split(".")[0]], layer_uid_of(key), eids.numpy(), dd, spec["msg_p"]))
        return masks[k]

    res, times = {}, {}
    for tag, dt in dtypes:
        t0 = time.time()
        P, _ = vae_cpu.split_state({k: (v.to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, names)
        opt = torch.optim.SGD([P[n] for n in names], lr=0.0)
        keep_mask = (lambda key, eids, dd, _dt=dt: keep(key, eids, dd).to(_dt)) if spec["msg_p"] > 0 else None
        with (vae_cpu.chunked_aggregation(chunk, device) if chunk is not None else contextlib.nullcontext()):
            outs, parts, grads = vae_cpu.train_step(_as_dtype(cpu, dt), P, names, cfg, opt, eps.to(dt), msg_dropout=spec["msg_p"],
                                                    keep_mask=keep_mask)
        res[tag] = (dict(zip(("s_logits", "c_logits", "mu", "log_var"), (o.detach() for o in outs))),
                    {k: float(v.detach()) for k, v in parts.items()}, grads)
        if states is not None:
            states[tag] = {k: v.detach().clone() for k, v in P.items() if k not in names and ".nn." not in k}
        times[tag] = time.time() - t0
    return res, times


def grad_errors(names, hip_g, g64, g32=None):
    """Per-tensor and whole-vector gradient errors against the fp64 oracle: per tensor max|a-b| over
    max(max|ref|, 1 % of the largest gradient) (the metric of tests/test_model_gpu._grad_err), and the relative L2 error
    of the concatenated gradient."""
    live = [n for n in names if g64[n] is not None]
    gmax = max(float(g64[n].abs().max()) for n in live)
    pairs = {"hip_vs_o64": (hip_g, g64)}
    if g32 is not None:
        pairs["o32_vs_o64"] = (g32, g64)
        pairs["hip_vs_o32"] = (hip_g, g32)
    worst = {t: (0.0, "") for t in pairs}
    num = {t: 0.0 for t in pairs}
    per_tensor, den2 = [], 0.0
    for n in live:
        c = g64[n].double()
        den = max(float(c.abs().max()), 1e-2 * gmax)
        for tag, (xa, ya) in pairs.items():
            x, y = xa[n].double(), ya[n].double()
            e = float((x - y).abs().max()) / den
            if e > worst[tag][0]:
                worst[tag] = (e, n)
            if tag == "hip_vs_o64":
                per_tensor.append((e, n, float(c.abs().max()) / gmax))
            num[tag] += float(((x - y) ** 2).sum())
        den2 += float((c ** 2).sum())
    for n in names:
        if g64[n] is None and hip_g[n] is not None:
            assert float(hip_g[n].abs().max()) == 0.0, n
    out = {tag: {"worst_tensor_err": worst[tag][0], "worst_tensor": worst[tag][1], "rel_l2": (num[tag] / den2) ** 0.5}
           for tag in pairs}
    out["gmax"] = gmax
    out["hip_worst_tensors"] = [{"err": round(e, 6), "tensor": n, "scale_vs_gmax": round(sc, 5)} for e, n, sc in sorted(per_tensor, reverse=True)[:10]]
    out["per_tensor"] = {n: e for e, n, _ in per_tensor}
    return out


def hip_vs_oracle_fullsize(spec, threads=None, dev="cuda"):
    """One native HIP training step (the measured variant) and the same step through oracle/vae_cpu.py in fp32 and in
    fp64 (same weights, eps and — replayed from the counter hash — the same message-dropout mask).  Returns the
    relative errors (max|a-b| / max|b|) of every model output, loss and of the gradient against the fp64 oracle, for
    both the HIP path and the fp32 oracle: the fp32 reference arithmetic is itself only defined up to its distance
    from fp64, which is what the tolerances of the full-size tests are measured against."""
    if threads:
        torch.set_num_threads(threads)
    run = hip_fullsize_step(spec, dev)
    cpu, names, got_l, hip, hip_g, info = (run[k] for k in ("cpu", "names", "losses", "outputs", "grads", "info"))
    S = info["n_slots"]
    res, times = oracle_fullsize(spec, run)
    o64, l64, g64 = res["o64"]
    o32, l32, g32 = res["o32"]
    rep = {"info": info, "N": cpu.num_nodes, "E": int(cpu.edge_index.shape[1]), "seconds": {"hip_first_step": run["seconds"], **times},
           "outputs": {}, "losses": {}, "grad": {}}
    for k in ("s_logits", "c_logits", "mu", "log_var"):
        ref64 = o64[k][:, :S] if k == "c_logits" else o64[k]
        ref32 = o32[k][:, :S] if k == "c_logits" else o32[k]
        rep["outputs"][k] = {"hip_vs_o64": rel_err(hip[k], ref64), "o32_vs_o64": rel_err(ref32, ref64), "hip_vs_o32": rel_err(hip[k], ref32)}
    for k in ("pitch", "dur", "structure", "kld"):
        den = max(1.0, abs(l64[k]))
        rep["losses"][k] = {"hip_vs_o64": abs(got_l[k] - l64[k]) / den, "o32_vs_o64": abs(l32[k] - l64[k]) / den}
    rep["grad"] = grad_errors(names, hip_g, g64, g32)
    rep["grad"].pop("per_tensor")
    return rep


# ---- the ReLU decisions a native step took, as masks for the oracle (oracle/kinks.ReluProbe.forced) ------------------------
SAVED = {k: i for i, k in enumerate(["GCN_H", "GCN_X", "GCN_XIN", "GCN_MEAN", "GCN_VAR", "GCN_T", "X0", "MERGE_PRE", "MERGE_MEAN",
                                     "MERGE_VAR", "DEC_PRE", "DEC_MEAN", "DEC_VAR", "ENC_CNN_LIN1"])}   # PM_SAVED_* of the header


def saved_tensor(step, what: str, stack: int = 0, layer: int = 0) -> torch.Tensor:
    """An activation of the last native forward, as a view of the step's workspace arena (pm_vae_step_saved)."""
    import ctypes
    from polyphemus_amd._lib import call
    off, n = ctypes.c_int64(), ctypes.c_int64()
    call("pm_vae_step_saved", step.addr, SAVED[what], stack, layer, ctypes.addressof(off), ctypes.addressof(n))
    return step.ws[off.value:off.value + 4 * n.value].view(torch.float32)


class LazyMsgDecisions:
    """The decisions of one message ReLU site, evaluated on demand: (x[src] * T[dist]) > 0 over the rows (positions in the
    relation's edge list) asked for, from the layer input and distance table the step saved (copied out of its arena) —
    what oracle/kinks.ReluProbe.forced takes in place of a materialised [E_r, d] mask."""

    def __init__(self, x, T, src, dist):
        self.x, self.T, self.src, self.dist = x, T, src, dist
        self.shape = torch.Size((src.shape[0], x.shape[1]))

    def __call__(self, rows):
        rows = rows.to(self.src.device)
        return (self.x.index_select(0, self.src[rows]) * self.T.index_select(0, self.dist[rows])) > 0


def hip_relu_decisions(live, cfg, lazy=False):
    """The ReLU decisions the BACKWARD of the native step just run on `live` (hip_fullsize_step(..., lr=0, keep=live)) took,
    keyed by the oracle's site index (oracle/kinks.relu_sites): per GCL layer the six per-relation message ReLUs
    (x[src] * T[dist] > 0 from the saved layer input and distance table: segreduce.hip k_segreduce_bwd) and the ReLU behind the
    norm (pm_bn_relu_decisions = the expression of pm_bn_bwd_elem on the saved pre-norm rows and batch statistics), the chord
    encoder's ReLU (its saved output > 0: pm_relu_bwd), the two head norms, CNNEncoder.lin[1].  Not imposed: the two
    BatchNorm2d ReLUs and the max-pool of the structure encoder's convolutions (0.8 M elements against 67 M), the structure
    decoder (the reference's loss sends no gradient there).  lazy=True: the message sites as LazyMsgDecisions over copies
    (on the device) of each layer's saved input and of the distance tables — 32 MB per layer at N = 16,384, d = 512, where
    the materialised masks would take 1 GB per layer."""
    import ctypes
    from oracle import kinks
    from polyphemus_amd._lib import call, ptr, stream
    vae, tr, g = live["vae"], live["trainer"], live["batch"]
    step = tr.step
    sites = kinks.relu_sites(cfg)
    N, d, L = g.num_nodes, cfg["d"], cfg["gnn_n_layers"]
    P = dict(vae.named_parameters())
    forced = {}

    def bn_mask(x, mean, var, key, rows, C):
        out = torch.empty(rows, C, dtype=torch.uint8, device=x.device)
        call("pm_bn_relu_decisions", ptr(x), ptr(mean), ptr(var), ptr(P[key + ".weight"].detach()), ptr(P[key + ".bias"].detach()),
             1e-5, rows, C, ptr(out), stream())
        return out.bool().cpu()

    et, ed, src = g.edge_type.long(), g.edge_dist.long(), g.edge_index[0].long()
    for stack, (tag, key) in enumerate((("enc_gcn", "encoder.c_encoder.graph_encoder"), ("dec_gcn", "decoder.c_decoder.graph_decoder"))):
        T = saved_tensor(step, "GCN_T", stack).view(32, d)
        if lazy:
            T = T.clone()
        for i in range(L):
            x = saved_tensor(step, "GCN_XIN", stack, i).view(N, d)
            if lazy:
                x = x.clone()
            for r in range(6):
                m = et == r
                forced[sites.index(f"{tag}.{i}.msg.{r}")] = (LazyMsgDecisions(x, T, src[m], ed[m]) if lazy else
                                                             ((x[src[m]] * T[ed[m]]) > 0).cpu())
            forced[sites.index(f"{tag}.{i}.norm")] = bn_mask(saved_tensor(step, "GCN_H", stack, i), saved_tensor(step, "GCN_MEAN", stack, i),
                                                             saved_tensor(step, "GCN_VAR", stack, i), f"{key}.norm_layers.{i}.module", N, d)
    x0 = saved_tensor(step, "X0").view(N, d) > 0
    drum = g.is_drum.bool()
    forced[sites.index("enc_chord.drums")] = x0[drum].cpu()
    forced[sites.index("enc_chord.non_drums")] = x0[~drum].cpu()
    B = g.s_tensor.shape[0] // cfg["n_bars"]
    forced[sites.index("enc_merge")] = bn_mask(saved_tensor(step, "MERGE_PRE"), saved_tensor(step, "MERGE_MEAN"),
                                               saved_tensor(step, "MERGE_VAR"), "encoder.bn_linear_merge", B, d)
    forced[sites.index("dec_bn")] = bn_mask(saved_tensor(step, "DEC_PRE"), saved_tensor(step, "DEC_MEAN"), saved_tensor(step, "DEC_VAR"),
                                            "decoder.batch_norm", B, 2 * d)
    forced[sites.index("enc_cnn.lin1")] = (saved_tensor(step, "ENC_CNN_LIN1").view(-1, d) > 0).cpu()
    torch.cuda.synchronize()
    return forced


# ---- eval mode under a trained-like BatchNorm state (tests/golden/<case>_evalstate.npz, oracle/make_golden.py evalstate) ----
def load_evalstate(case):
    """(golden case, cfg, evalstate fixture, state dict): the case's initial state with the fixture's BatchNorm tensors
    (weight, bias, running statistics, num_batches_tracked of every norm) in place."""
    z, cfg = load_case(case)
    ze = np.load(os.path.join(GOLDEN, f"{case}_evalstate.npz"), allow_pickle=False)
    sd = state_dict_from_golden(z)
    for k in ze.files:
        if k.startswith("bn/"):
            assert k[3:] in sd, k
            sd[k[3:]] = torch.from_numpy(ze[k].copy())
    return z, cfg, ze, sd


def bn_keys(sd):
    """The prefixes of every BatchNorm of a state dict, in key order."""
    return [k[:-len(".running_mean")] for k in sd if k.endswith(".running_mean")]


def oracle_structure_logits(z, P, cfg):
    """The structure half of `Decoder.forward` in eval mode (model.py:634-645) through oracle/vae_cpu.py: what the
    generation path thresholds before any graph exists."""
    import torch.nn.functional as F
    from oracle import vae_cpu
    h = F.relu(vae_cpu._bn(vae_cpu._lin(z, P, "decoder.lin_decoder"), P, "decoder.batch_norm", False))
    return vae_cpu.structure_decoder(h[:, :cfg["d"]], P, cfg, False)


def host_graph_from_binary(s_bin, n_bars):
    """The batch of bar graphs of a binary structure [B, n_bars, 4, 32], built by the host builder
    (polyphemus_amd/graphs.py, the reference's `graph_from_tensor` per sample) on the CPU."""
    from polyphemus_amd.graphs import collate_samples, graph_from_structure
    s_np = s_bin.detach().cpu().numpy().astype(bool)
    samples = []
    for i in range(s_np.shape[0]):
        g = graph_from_structure(s_np[i])
        g["tokens"] = np.zeros((g["num_nodes"], 16, 2), np.int32)
        g["s_tensor"] = s_np[i].astype(np.float32)
        samples.append(g)
    return collate_samples(samples, n_bars)


def trained_like_state(spec, dev="cuda", n_fill=20, seed=4321):
    """A trained-like state of the `spec` model (its FULLSIZE configuration): the default init under manual_seed(0), running
    statistics filled by `n_fill` training-mode no_grad forwards of the Python path on synthetic batches of seeds
    seed, seed + 1, ... (momentum 0.1: 1 - 0.9^20 = 88 % of the batch statistics), then every norm's weight
    = 1 + 0.5 U(-1, 1) and bias = 0.3 N(0, 1) from torch.Generator().manual_seed(seed).  Returns (cfg, state dict on the
    CPU).  What the forwards compute does not matter to a comparison: the oracle is given the same state dict."""
    from polyphemus_amd.model import VAE
    from polyphemus_amd.synthetic import synthetic_batch
    cfg = dict(dropout=0, batch_norm=True, gnn_n_layers=spec["L"], d=spec["d"], n_bars=spec["nb"], resolution=8)
    torch.manual_seed(0)
    vae = VAE(**cfg, device=dev).to(dev)
    vae.train()
    with torch.no_grad():
        for i in range(n_fill):
            vae(synthetic_batch(spec["B"], spec["nb"], p=spec["p"], seed=seed + i, dense=spec["dense"]).to(dev))
    sd = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    del vae
    gen = torch.Generator().manual_seed(seed)
    for k in bn_keys(sd):
        w = sd[k + ".weight"]
        sd[k + ".weight"] = 1 + 0.5 * (2 * torch.rand(w.shape, generator=gen) - 1)
        sd[k + ".bias"] = 0.3 * torch.randn(w.shape, generator=gen)
    return cfg, sd


def content_correct(c_logits, tokens):
    """Per (node, slot 1..15) row: (pitch arg-max == target, duration arg-max == target, pitch target not PAD, duration
    target not PAD) — the element-wise terms of `_accuracies` (training.py:349-468), bool [N, 15] each."""
    from polyphemus_amd import constants as C
    c = c_logits.detach().cpu()
    t = tokens.detach().cpu().long()[:, 1:]
    p_ok = c[..., :C.N_PITCH_TOKENS].argmax(-1) == t[..., 0]
    d_ok = c[..., C.N_PITCH_TOKENS:].argmax(-1) == t[..., 1]
    return p_ok, d_ok, t[..., 0] != C.PITCH_PAD, t[..., 1] != C.DUR_PAD


def top2_margin(c_logits):
    """Per (node, slot) row: the smaller of the pitch and duration top-1 / top-2 logit margins (float64 [N, 15])."""
    from polyphemus_amd import constants as C
    c = c_logits.detach().double().cpu()
    m = []
    for part in (c[..., :C.N_PITCH_TOKENS], c[..., C.N_PITCH_TOKENS:]):
        top = part.topk(2, dim=-1).values
        m.append(top[..., 0] - top[..., 1])
    return torch.minimum(*m)


def oracle_eval_fullsize(cfg, cpu, sd, names, eps, dtypes=(("o64", torch.float64), ("o32", torch.float32))):
    """The eval-mode entry of the full-size oracle: oracle/vae_cpu.py's forward with training=False (running statistics,
    no dropout of any kind) on the CPU batch `cpu`, the state dict `sd` and `eps`, per dtype: (outputs, the 7 losses as
    floats, the state the forward left), and the seconds each took."""
    import time
    from oracle import vae_cpu
    res, times = {}, {}
    for tag, dt in dtypes:
        t0 = time.time()
        P, _ = vae_cpu.split_state({k: (v.to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, names)
        b = _as_dtype(cpu, dt)
        with torch.no_grad():
            (s_logits, c_logits), mu, lv = vae_cpu.vae_forward(b, P, cfg, False, eps.to(dt))
            _, parts = vae_cpu.losses(b.s_tensor, s_logits, b.c_tensor, c_logits, mu, lv)
        res[tag] = (dict(s_logits=s_logits, c_logits=c_logits, mu=mu, log_var=lv), {k: float(v) for k, v in parts.items()},
                    {k: v.detach() for k, v in P.items()})
        times[tag] = time.time() - t0
    return res, times


def assert_eval_c_logits_match(c_logits, ze, tol, argmax_mismatch):
    """Eval c_logits [N, 15, 230] against an evalstate fixture, to `tol` of max|c_logits| per logit: every node's logits of
    the stored slots (eval/c_logits_slots, where the fixture has them), per (node, slot) sums (|error| <= 230 tol max) and
    L2 norms (<= sqrt(230) tol max), per-node sums; arg-max tokens differing at no more than `argmax_mismatch` of them."""
    from polyphemus_amd import constants as C
    c = c_logits.detach().cpu()
    m = float(c.abs().max())
    if "eval/c_logits_slots" in ze.files:
        want = ze["eval/c_logits_slots"]
        assert rel_err(c[:, :want.shape[1]], want) < tol, "c_logits slots"
    cd = c.double()
    assert float(np.abs(cd.sum(-1).numpy() - ze["eval/c_logits_slotsum"]).max()) < tol * m * C.D_TOKEN_PAIR, "slot sums"
    assert float(np.abs(cd.norm(dim=-1).numpy() - ze["eval/c_logits_slotnorm"]).max()) < tol * m * C.D_TOKEN_PAIR ** 0.5, \
        "slot norms"
    assert float(np.abs(cd.sum(dim=(-1, -2)).numpy() - ze["eval/c_logits_nodesum"]).max()) < tol * m * C.N_SLOTS * C.D_TOKEN_PAIR
    tok = torch.stack([c[..., :C.N_PITCH_TOKENS].argmax(-1), c[..., C.N_PITCH_TOKENS:].argmax(-1)], -1).numpy()
    assert (tok != ze["eval/c_argmax"]).mean() <= argmax_mismatch, "arg-max tokens"
