"""The self block of the compact aggregate A' = [track | onset | next | x] without its round trip through HBM.

Columns [3d, 4d) of the A' planes are the split of the layer's own input row (pair format: of x[n] times the plane scale).  The
fused forward can leave them unwritten (`pm_gcl_forward_fused_sel` / `_sel_h2` with self_planes = 0) and the tile weight gradient
can take those rows from x itself (`pm_gcl_weight_grad_fused_x` / `_x_h2`); the step does both unless PM_GCL_SELF_PLANES=1.

    forward          the self columns of every plane keep a pre-filled bit pattern; every other column, h and the plane scale are
                     bit-equal to the entry that stores all four blocks; in deterministic mode the norm's column sums too
    weight gradient  A' planes whose self columns hold NaN patterns + x give the dW of the full planes: `torch.equal` in
                     deterministic mode, both within 2e-6 of the fp64 product's largest term otherwise (the bound of
                     test_gcl_weight_grad_fused_equals_grouped_product), accumulating into a non-zero dW
    step             losses and the whole gradient of the native step, bit for bit, under PM_GCL_SELF_PLANES=0 and =1

Shapes: two bars, B = 2 / 8 (118 / 502 nodes: no multiple of 32, one and several row tiles per track group; at d = 128 the
weight gradient's sixteen K slices leave workgroups without rows) and a batch whose fourth track has no node; d = 128, 256
(gcl.hip) and 512 (wide.hip forward); both operand formats; message dropout 0 and 0.1; row classes on and off."""
import ctypes

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib, ops
from polyphemus_amd._lib import call, ptr, stream
from polyphemus_amd.graphs import collate_samples
from polyphemus_amd.synthetic import disk_sample, sample_from_disk, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = 0x5A5A                 # what the planes hold before the forward writes them
NAN_BITS = {"triple": 0x7FC0, "pair": 0x7E00}          # a quiet NaN of the plane type (bf16 / fp16)
WS = 16.0                        # scale of the pair format's weight planes
SEED, LAYER = 5, 2


class _PmH2(ctypes.Structure):
    _fields_ = [("absmax_in", ctypes.c_void_p), ("absmax_aux", ctypes.c_void_p), ("scale_out", ctypes.c_void_p),
                ("w_scale", ctypes.c_float), ("reserved", ctypes.c_int32)]


def _batch_without_track(B, seed, track=3):
    """`synthetic_batch` with one track silent in every sample: its track group has no node"""
    rng = np.random.default_rng(seed)
    samples = []
    for _ in range(B):
        c, s = disk_sample(rng, 2, 0.25)
        s[track, :] = False
        samples.append(sample_from_disk(c, s, 2))
    return collate_samples(samples, 2)


_CASES = {}


def _case(name, d):
    """(plan, N, x, T, W, bias) of a batch and a width: built once, shared by the tests, never written"""
    if (name, d) not in _CASES:
        if name not in _CASES:
            cpu = {"b2": lambda: synthetic_batch(2, 2, p=0.25, seed=41), "b8": lambda: synthetic_batch(8, 2, p=0.25, seed=41),
                   "empty": lambda: _batch_without_track(8, 41)}[name]()
            b = cpu.to(DEV)
            plan = ops.plan_build(b.edge_index, b.edge_type, b.edge_dist, b.bars, b.batch, b.is_drum, b.tokens, b.n_bars,
                                  b.s_tensor.shape[0])
            _CASES[name] = (b, plan, cpu.num_nodes)
        b, plan, N = _CASES[name]
        assert N % 32 != 0
        if name == "empty":
            assert int((plan.field("trk_cnt")[:4] == 0).sum()) == 1 and int(plan.field("trk_cnt")[:4].sum()) == N
        g = torch.Generator(device="cpu").manual_seed(1000 + d)
        rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
        x = rn(N, d) * 3.0
        T = ops.edge_table(rn(d, 32) * 0.5, rn(d) * 0.1)
        W = rn(7 * d, d) / d ** 0.5
        bias = rn(d)
        _CASES[(name, d)] = (plan, N, x, T, W, bias)
    return _CASES[(name, d)]


def _weights(W, d, fmt):
    Wf = ops.split_planes_frag(W, 1)
    if fmt == "pair":
        Wf2 = torch.zeros_like(Wf)
        call("pm_split_planes_frag_h2", ptr(W), 7 * d, d, 1, 1, 7 * d * d, 7 * d * d * 3, WS, ptr(Wf2), stream())
        return Wf2
    return Wf


def _absmax_words(t):
    w = torch.zeros(64, dtype=torch.int32, device=t.device)
    call("pm_absmax", ptr(t), t.numel(), ptr(w), stream())
    return w


def _forward(case, d, fmt, p, use_classes, Wf, planes, self_planes, stats):
    """one forward call: self_planes None = the entry that stores all four blocks; 0 / 1 = the new entry.  -> (h, plane scale)"""
    plan, N, x, T, W, bias = case
    h = torch.empty(N, d, device=DEV)
    sA = torch.zeros(1, device=DEV)
    head = (ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, p, SEED, LAYER, ptr(Wf), ptr(bias), use_classes, ptr(h), ptr(stats),
            ptr(planes), N * 4 * d)
    if fmt == "pair":
        mx, mt = _absmax_words(x), _absmax_words(T)
        hh = _PmH2(ptr(mx), ptr(mt), ptr(sA), WS, 0)
        if self_planes is None:
            call("pm_gcl_forward_fused_h2", *head, ctypes.addressof(hh), stream())
        else:
            call("pm_gcl_forward_fused_sel_h2", *head, ctypes.addressof(hh), self_planes, stream())
        torch.cuda.synchronize()                # (hh and the |max| words live until the kernel has run)
    elif self_planes is None:
        call("pm_gcl_forward_fused", *head, stream())
    else:
        call("pm_gcl_forward_fused_sel", *head, self_planes, stream())
    return h, sA


def _filled(N, d, value):
    return torch.full((3, N * 4 * d), value, dtype=torch.int16, device=DEV)


def _decode(planes, fmt, scale=1.0):
    """int16 planes -> the fp64 values they stand for"""
    if fmt == "pair":
        return (planes[0].view(torch.float16).double() + planes[1].view(torch.float16).double()) / scale
    f = lambda t: (t.to(torch.int32) << 16).view(torch.float32).double()
    return f(planes[0]) + f(planes[1]) + f(planes[2])


@pytest.mark.parametrize("name", ["b2", "b8", "empty"])
@pytest.mark.parametrize("fmt", ["pair", "triple"])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_forward_leaves_the_self_block_unwritten_and_everything_else_alone(d, fmt, name):
    case = _case(name, d)
    plan, N, x, T, W, bias = case
    Wf = _weights(W, d, fmt)
    for det in (False, True):
        for p in (0.0, 0.1):
            for use_classes in (1, 0):
                with _lib.deterministic(det):
                    s_old = torch.zeros(8, 2, d, dtype=torch.float64, device=DEV)
                    s_new = torch.zeros_like(s_old)
                    P_old, P_new = _filled(N, d, PATTERN), _filled(N, d, PATTERN)
                    h_old, sa_old = _forward(case, d, fmt, p, use_classes, Wf, P_old, None, s_old)
                    h_new, sa_new = _forward(case, d, fmt, p, use_classes, Wf, P_new, 0, s_new)
                    torch.cuda.synchronize()
                tag = (det, p, use_classes)
                v_old, v_new = P_old.view(3, N, 4 * d), P_new.view(3, N, 4 * d)
                assert bool((v_new[:, :, 3 * d:] == PATTERN).all()), tag
                assert torch.equal(v_new[:, :, :3 * d], v_old[:, :, :3 * d]), tag
                assert torch.equal(h_new, h_old) and torch.equal(sa_new, sa_old), tag
                if det:
                    assert torch.equal(s_new, s_old), tag
                else:
                    assert float((s_new.sum(0) - s_old.sum(0)).abs().max()) <= 1e-9 * float(s_old.sum(0).abs().max()), tag
                # what is no longer stored is the split of x (times the plane scale): the weight gradient can rebuild it
                sc = float(sa_old) if fmt == "pair" else 1.0
                self_old = _decode(v_old[:, :, 3 * d:].reshape(3, -1), fmt, sc).view(N, d)
                if fmt == "triple":
                    assert torch.equal(self_old, x.double()), tag
                else:
                    assert float((self_old - x.double()).abs().max()) <= 2.0 ** -21 * float(x.abs().max()), tag
    # self_planes != 0: the entry that stores all four blocks
    P_old, P_new = _filled(N, d, PATTERN), _filled(N, d, PATTERN)
    h_old, sa_old = _forward(case, d, fmt, 0.1, 1, Wf, P_old, None, None)
    h_new, sa_new = _forward(case, d, fmt, 0.1, 1, Wf, P_new, 1, None)
    assert torch.equal(P_new, P_old) and torch.equal(h_new, h_old) and torch.equal(sa_new, sa_old)


def _pair_planes(v, scale):
    """fp32 values -> [3, n] int16 planes in the fp16 pair format (hi, lo, unused)"""
    w = v.reshape(-1) * scale
    hi = w.half()
    lo = (w - hi.float()).half()
    return torch.stack([hi.view(torch.int16), lo.view(torch.int16), torch.zeros_like(hi).view(torch.int16)]).contiguous()


@pytest.mark.parametrize("name", ["b2", "b8", "empty"])
@pytest.mark.parametrize("fmt", ["pair", "triple"])
@pytest.mark.parametrize("d", [128, 256, 512])
def test_weight_gradient_takes_the_self_block_from_x(d, fmt, name):
    case = _case(name, d)
    plan, N, x, T, W, bias = case
    Wf = _weights(W, d, fmt)
    g = torch.Generator(device="cpu").manual_seed(7 + d)
    dh = torch.randn(N, d, generator=g).to(DEV)
    base = torch.randn(7 * d, d, generator=g).to(DEV)             # dW accumulates: it starts non-zero
    sdh = torch.full((1,), 2.0 ** 10, device=DEV)
    dhp = _pair_planes(dh, float(sdh)) if fmt == "pair" else ops.split_planes(dh)
    trel = plan.field("node_trel").long()[:N]
    for p in (0.0, 0.1):
        full = _filled(N, d, 0)                                    # (blocks a row class does not write are zero aggregates)
        _, sA = _forward(case, d, fmt, p, 1, Wf, full, None, None)
        holes = full.clone()
        holes.view(3, N, 4 * d)[:, :, 3 * d:] = NAN_BITS[fmt]
        assert bool(torch.isnan(holes.view(3, N, 4 * d)[0, :, 3 * d:].view(torch.float16 if fmt == "pair" else torch.bfloat16)).all())
        A = _decode(full, fmt, float(sA) if fmt == "pair" else 1.0).view(N, 4 * d)
        dhv = _decode(dhp, fmt, float(sdh) if fmt == "pair" else 1.0).view(N, d)
        want = base.double().clone()
        for t in range(4):
            rows = trel == t
            want[t * d:(t + 1) * d] += A[rows, :d].T @ dhv[rows]
        want[4 * d:] += A[:, d:].T @ dhv
        scale = float((want - base.double()).abs().max())

        def run(planes, xin, use_classes):
            dW = base.clone()
            head = (ptr(planes), N * 4 * d) + ((ptr(xin),) if xin is not None else ()) + \
                   (ptr(dhp), N * d, ptr(plan.buf), N, plan.E, plan.G, d, use_classes, ptr(dW))
            sfx = ("_x" if xin is not None else "") + ("_h2" if fmt == "pair" else "")
            if fmt == "pair":
                call("pm_gcl_weight_grad_fused" + sfx, *head, ptr(sA), ptr(sdh), stream())
            else:
                call("pm_gcl_weight_grad_fused" + sfx, *head, stream())
            return dW

        for use_classes in (1, 0):
            for det in (False, True):
                with _lib.deterministic(det):
                    dW_old = run(full, None, use_classes)
                    dW_new = run(holes, x, use_classes)
                    torch.cuda.synchronize()
                tag = (p, use_classes, det)
                e_old, e_new = float((dW_old.double() - want).abs().max()), float((dW_new.double() - want).abs().max())
                print(f"d={d} {fmt} {name} {tag}: |dW - fp64|max / scale  old {e_old / scale:.3e}  new {e_new / scale:.3e}")
                assert bool(torch.isfinite(dW_new).all()), tag
                if det:
                    assert torch.equal(dW_new, dW_old), tag
                assert e_old < 2e-6 * scale and e_new < 2e-6 * scale, (tag, e_old / scale, e_new / scale)


def test_weight_gradient_refuses_rows_beyond_32_bit_offsets():
    """N * d * 4 >= 2^31: PM_E_INVALID before anything is launched (the pointers are never dereferenced)"""
    t = torch.zeros(64, device=DEV)
    N, d = (1 << 20) + 1, 512
    rc = _lib.lib().pm_gcl_weight_grad_fused_x(ptr(t), N * 4 * d, ptr(t), ptr(t), N * d, ptr(t), N, 0, 1, d, 1, ptr(t), stream())
    assert rc == -1


@pytest.mark.parametrize("d,dropout", [(128, 0), (256, 0), (256, 0.1)])
def test_step_is_bit_identical_with_and_without_the_stored_self_block(d, dropout):
    """The native step (B = 8, L = 2, message dropout 0.1; with the model's dropout the weight gradient reads the dropped copy)
    in deterministic mode: PM_GCL_SELF_PLANES=1 (the self block stored and read back) against the default."""
    import os
    from util import hip_fullsize_step
    spec = dict(B=8, nb=2, L=2, p=0.25, dense=False, msg_p=0.1, seed=1234, d=d, dropout=dropout)

    def switch(v):
        if v is None:
            os.environ.pop("PM_GCL_SELF_PLANES", None)
        else:
            os.environ["PM_GCL_SELF_PLANES"] = str(v)
        assert _lib.lib().pm_vae_step_reload_switches() == 0

    prev = os.environ.get("PM_GCL_SELF_PLANES")
    try:
        with _lib.deterministic(True):
            switch(0)
            a = hip_fullsize_step(spec, lr=0.0)
            switch(1)
            b = hip_fullsize_step(spec, lr=0.0)
    finally:
        switch(prev)
    assert a["info"]["launches"]["gcl_fwd"] == 4 and a["info"]["launches"]["gcl_dw"] == 4, a["info"]
    assert a["info"]["launches"] == b["info"]["launches"]
    assert a["losses"] == b["losses"]
    for k in a["names"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    assert sum(float(v.abs().max()) > 0 for v in a["grads"].values()) >= 50
