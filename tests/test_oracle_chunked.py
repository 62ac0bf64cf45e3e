"""The edge-chunked GCL aggregation of the oracle (oracle/vae_cpu.chunked_aggregation: what lets the fp64 oracle run one
GPU's configs[4] shard at its real size) against the default per-relation path it restates, the torch restatement of the
dropout counter hash it replays message dropout from, and lazily imposed ReLU decisions (oracle/kinks.ReluProbe.forced
with callables) against materialised ones.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import kinks, vae_cpu
from polyphemus_amd import _lib
from polyphemus_amd.model import VAE
from polyphemus_amd.synthetic import synthetic_batch
from util import (LazyMsgDecisions, _as_dtype, batch_from_golden, dropout_hash_torch, dropout_keep_np, dropout_keep_torch,
                  layer_uid_of, load_case, rel_err, state_dict_from_golden)

D = 32
KEY = "encoder.c_encoder.graph_encoder.layers.1"


@pytest.fixture(scope="module")
def params():
    """fp64 leaf parameters of a d = 32 model: the GCL layer under test is KEY (its edge network is shared with layer 0)"""
    torch.manual_seed(0)
    vae = VAE(dropout=0, batch_norm=True, gnn_n_layers=2, d=D, n_bars=2, resolution=8, device=torch.device("cpu"))
    sd = {k: v.detach().double() if v.dtype.is_floating_point else v.clone() for k, v in vae.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    for k in (KEY + ".bias", KEY + ".root", KEY + ".weight"):          # zero-init biases: make every term count
        sd[k] = sd[k] + 0.1 * torch.randn(sd[k].shape, generator=g, dtype=torch.float64)
    names = [n for n, _ in vae.named_parameters()]
    return vae_cpu.split_state(sd, names)[0]


def _graph(kind):
    if kind == "sparse":
        b = synthetic_batch(4, 2, p=0.25, seed=5)
    elif kind == "dense":
        b = synthetic_batch(1, 2, p=1.0, seed=3, dense=True)
    else:                                                               # relation 2 has no edge at all
        b = synthetic_batch(4, 2, p=0.25, seed=5)
    ea = b.edge_attrs.double()
    ei = b.edge_index
    if kind == "empty_relation":
        m = ea[:, 0] != 2
        ea, ei = ea[m], ei[:, m]
    return ei, ea[:, 0], ea[:, 1:], b.num_nodes


def _keep(p):
    def keep(key, eids, dd):
        return dropout_keep_torch(77, layer_uid_of(key), eids, dd, p).double()
    return keep


def _run(path, P, ei, et, ea, N, p, chunk):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, D, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(N, D, generator=g, dtype=torch.float64)
    leaves = [x] + [P[KEY + s] for s in (".nn.weight", ".nn.bias", ".weight", ".root", ".bias")]
    for t in leaves[1:]:
        t.grad = None
    if path == "default":
        y = vae_cpu.gcl_forward(x, ei, et, ea, P, KEY, True, p, _keep(p) if p > 0 else None)
    else:
        y = vae_cpu.gcl_forward_chunked(x, vae_cpu.gcl_edges(ei, et, ea, N, x.dtype), ea.shape[1], P, KEY, True, p,
                                        _keep(p) if p > 0 else None, chunk=chunk)
    (y * gy).sum().backward()
    return [y.detach()] + [t.grad.clone() for t in leaves]


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("kind,chunk", [("sparse", 1), ("sparse", 97), ("sparse", 10 ** 6), ("dense", 4099), ("dense", 10 ** 6),
                                        ("empty_relation", 13)])
def test_chunked_aggregation_is_gcl_forward(params, kind, chunk, p):
    """forward and dx, d nn.weight, d nn.bias, d W_r, d root, d bias of the chunked layer = those of gcl_forward in fp64,
    for chunks of one edge, chunks that do not divide any relation's edge count and one chunk larger than every relation"""
    ei, et, ea, N = _graph(kind)
    if kind == "empty_relation":
        assert int((et == 2).sum()) == 0 and int((et == 3).sum()) > 0
    want = _run("default", params, ei, et, ea, N, p, None)
    got = _run("chunked", params, ei, et, ea, N, p, chunk)
    for what, a, b in zip(("out", "dx", "d nn.weight", "d nn.bias", "d W_r", "d root", "d bias"), got, want):
        assert float(b.abs().max()) > 0, what
        assert rel_err(a, b) <= 1e-12, (what, rel_err(a, b))


def test_chunked_aggregation_requires_one_hot_distances(params):
    ei, et, ea, N = _graph("sparse")
    bad = ea.clone()
    bad[3, 0] += 0.5
    with pytest.raises(AssertionError, match="one-hot"):
        vae_cpu.gcl_edges(ei, et, bad, N, torch.float64)


def _assert_grads_agree(got, want, names, tol):
    """every gradient within `tol` of `want`'s, per tensor against max(its own scale, 1e-3 of the largest gradient): the
    gradients of the biases ahead of a BatchNorm are exactly zero, i.e. rounding noise at 1e-16 of the largest one, which
    another summation order changes completely"""
    live = [n for n in names if want[n] is not None]
    assert len(live) > 20 and all(got[n] is None for n in names if want[n] is None)
    gmax = max(float(want[n].abs().max()) for n in live)
    for n in live:
        err = float((got[n] - want[n]).abs().max()) / max(float(want[n].abs().max()), 1e-3 * gmax)
        assert err <= tol, (n, err)
    return live


def _golden_step(case, chunk, keep):
    z, cfg = load_case(case)
    names = [str(n) for n in z["param_names"]]
    sd = state_dict_from_golden(z)
    P, _ = vae_cpu.split_state({k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, names)
    opt = torch.optim.SGD([P[n] for n in names], lr=0.0)
    g = _as_dtype(batch_from_golden(z, cfg), torch.float64)
    eps = torch.from_numpy(z["in/eps"]).double()
    if chunk is None:
        return vae_cpu.train_step(g, P, names, cfg, opt, eps, msg_dropout=0.1, keep_mask=keep), names
    with vae_cpu.chunked_aggregation(chunk):
        return vae_cpu.train_step(g, P, names, cfg, opt, eps, msg_dropout=0.1, keep_mask=keep), names


@pytest.mark.parametrize("case", ["lmd2_tiny", "nb3_tiny"])
def test_golden_step_through_the_chunked_path(case):
    """The whole fp64 training step of a golden case with message dropout p = 0.1 (replayed from the counter hash) through
    the chunked aggregation: every output, loss and gradient equals the default path's to 1e-10."""
    keep = _keep(0.1)
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        (outs0, parts0, g0), names = _golden_step(case, None, keep)
        (outs1, parts1, g1), _ = _golden_step(case, 50, keep)
    finally:
        torch.set_num_threads(n)
    for a, b in zip(outs1, outs0):
        assert rel_err(a.detach(), b.detach()) <= 1e-10
    for k in parts0:
        a, b = float(parts1[k].detach()), float(parts0[k].detach())
        assert abs(a - b) <= 1e-10 * max(1.0, abs(b)), k
    _assert_grads_agree(g1, g0, names, 1e-10)


@pytest.mark.parametrize("case", ["lmd2_tiny", "nb3_tiny"])
def test_eval_forward_through_the_chunked_path(case):
    """eval mode through the chunked aggregation matches the reference's captured eval/* tensors (test_eval_forward's bound)"""
    z, cfg = load_case(case)
    g = batch_from_golden(z, cfg)
    P, _ = vae_cpu.split_state(state_dict_from_golden(z), [str(n) for n in z["param_names"]])
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad(), vae_cpu.chunked_aggregation(64):
            (s_logits, c_logits), mu, lv = vae_cpu.vae_forward(g, P, cfg, False, torch.from_numpy(z["in/eps"]))
    finally:
        torch.set_num_threads(n)
    for name, got in (("s_logits", s_logits), ("c_logits", c_logits), ("mu", mu), ("log_var", lv)):
        assert rel_err(got, z[f"eval/{name}"]) < 1e-6, name


def test_default_path_stays_the_default():
    assert vae_cpu.EDGE_CHUNK is None and vae_cpu.EDGE_DEVICE is None
    with vae_cpu.chunked_aggregation(8, "cpu"):
        assert vae_cpu.EDGE_CHUNK == 8
    assert vae_cpu.EDGE_CHUNK is None and vae_cpu.EDGE_DEVICE is None


# ---- the dropout counter hash in torch ------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_torch_dropout_hash_is_the_numpy_replica_and_the_librarys(p):
    """dropout_keep_torch = dropout_keep_np bit for bit (edge ids past 2^24 and 2^31, all 512 channels, seeds with the top
    bit set), and dropout_hash_torch = the library's pm_dropout_hash on sampled (seed, layer, edge, channel) tuples"""
    L = _lib.lib()
    rng = np.random.default_rng(int(p * 100))
    eids = np.concatenate([np.arange(300), rng.integers(1 << 24, 1 << 32, 300), [(1 << 24) - 1, 1 << 24, (1 << 24) + 1,
                                                                              (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 2080767]])
    for seed, uid in ((1234, 0), (0xFFFFFFFF, 1007), (0x80000001, 3), (99, 1000)):
        want = dropout_keep_np(seed, uid, eids, 512, p)
        got = dropout_keep_torch(seed, uid, torch.from_numpy(eids.astype(np.int64)), 512, p)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want), (seed, uid)
        assert abs(float(want.mean()) - (1 - p)) < 0.01
        h = dropout_hash_torch(seed, uid, torch.from_numpy(eids.astype(np.int64)), 512)
        thr = int(np.float32(p) * np.float32(16777216.0))
        for _ in range(64):
            i, c = int(rng.integers(0, eids.size)), int(rng.integers(0, 512))
            lib_h = L.pm_dropout_hash(seed, uid, int(eids[i]), c)
            assert int(h[i, c]) == lib_h, (seed, uid, int(eids[i]), c)
            assert (lib_h >= thr) == bool(want[i, c])
        for c in (0, 1, 2, 3, 4, 255, 508, 511):
            assert int(h[-2, c]) == L.pm_dropout_hash(seed, uid, int(eids[-2]), c)


# ---- lazily imposed ReLU decisions --------------------------------------------------------------------------------------
def test_lazy_msg_decisions_are_the_product_sign():
    g = torch.Generator().manual_seed(2)
    x, T = torch.randn(40, 16, generator=g), torch.randn(32, 16, generator=g)
    src, dist = torch.randint(0, 40, (300,), generator=g), torch.randint(0, 32, (300,), generator=g)
    lazy = LazyMsgDecisions(x, T, src, dist)
    rows = torch.tensor([0, 5, 299, 17])
    assert lazy.shape == (300, 16)
    assert torch.equal(lazy(rows), (x[src[rows]] * T[dist[rows]]) > 0)


@pytest.fixture(scope="module")
def small_case():
    cfg = dict(dropout=0, batch_norm=True, gnn_n_layers=2, d=D, n_bars=2, resolution=8)
    torch.manual_seed(0)
    vae = VAE(**cfg, device=torch.device("cpu"))
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    names = [n for n, _ in vae.named_parameters()]
    batch = synthetic_batch(4, 2, p=0.25, seed=5)
    eps = torch.randn(4, D, generator=torch.Generator().manual_seed(1))
    keep = _keep(0.1)
    _, _, probe, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, keep=True)
    sites = kinks.relu_sites(cfg)
    assert len(probe.pre) == len(sites)
    # decisions of every message site and of one norm site, with some inverted: the oracle's own sign everywhere else
    g = torch.Generator().manual_seed(4)
    forced = {}
    for i, name in enumerate(sites):
        if ".msg." in name or name == "dec_gcn.1.norm":
            m = probe.pre[i] > 0
            flip = torch.rand(m.shape, generator=g) < 0.02
            forced[i] = m ^ flip
    return cfg, sd, names, batch, eps, keep, sites, forced


class _Rows:
    """a callable message site over a materialised mask (what LazyMsgDecisions computes from the saved tensors)"""

    def __init__(self, m):
        self.m, self.calls = m, 0

    def __call__(self, rows):
        self.calls += 1
        return self.m[rows]


@pytest.mark.parametrize("chunk", [None, 1, 29])
def test_lazy_forced_decisions_are_the_materialised_ones(small_case, chunk):
    """The same gradient and the same per-site disagree counts whether a message site's decisions come as a tensor or as
    a callable, on the default path and on the chunked one (the chunked path accumulates the counts over its chunks)"""
    import contextlib
    cfg, sd, names, batch, eps, keep, sites, forced = small_case
    lazy = {i: (_Rows(m) if ".msg." in sites[i] else m) for i, m in forced.items()}
    g_mat, l_mat, p_mat, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, forced=forced)
    with (vae_cpu.chunked_aggregation(chunk) if chunk else contextlib.nullcontext()):
        g_lazy, l_lazy, p_lazy, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, forced=lazy)
    assert all(f.calls >= 1 for f in lazy.values() if isinstance(f, _Rows))
    assert set(p_lazy.disagree) == set(forced) and p_lazy.disagree == p_mat.disagree
    assert sum(p_mat.disagree.values()) > 100                     # the inverted decisions are seen as such
    assert p_lazy.count == p_mat.count == len(sites)
    for k in l_mat:
        assert abs(l_lazy[k] - l_mat[k]) <= 1e-10 * max(1.0, abs(l_mat[k])), k
    live = _assert_grads_agree(g_lazy, g_mat, names, 0.0 if chunk is None else 1e-10)
    g_own, _, _, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep)
    assert sum(rel_err(g_own[n], g_mat[n]) > 1e-3 for n in live) > 10     # the imposed decisions change the gradient


def test_chunked_probe_records_and_flips_like_the_default(small_case):
    """ReluProbe's other two uses through the chunked path: the recorded pre-activations and the single-flip gradients of
    kinks.kink_gradients (flat indices into a message site's [E_r, d])"""
    cfg, sd, names, batch, eps, keep, sites, _ = small_case
    _, _, p0, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, keep=True)
    with vae_cpu.chunked_aggregation(7):
        _, _, p1, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, keep=True)
    assert len(p0.pre) == len(p1.pre)
    for a, b in zip(p1.pre, p0.pre):
        assert a.shape == b.shape and (a.numel() == 0 or rel_err(a, b) <= 1e-12)
    site = sites.index("dec_gcn.0.msg.5")
    pre = p0.pre[site]
    idx = torch.nonzero(pre.reshape(-1) > 0).reshape(-1)[torch.tensor([0, 7, 40])]
    g0, _, _, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, flips={site: idx})
    with vae_cpu.chunked_aggregation(7):
        g1, _, _, _ = kinks._step(batch, sd, names, cfg, eps, 0.1, keep, flips={site: idx})
    _assert_grads_agree(g1, g0, names, 1e-10)
