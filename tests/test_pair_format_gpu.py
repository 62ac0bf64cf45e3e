"""The fp16 pair operand format (PmH2, include/polyphemus_hip.h) where a tensor's bulk lies far below its |max|.

Every other test of the format draws Gaussian operands, whose bulk sits 2^2 below their |max|.  One power-of-two scale
serves a whole tensor and the dh scale is a bound that is loose by design, so what limits the format is DYNAMIC RANGE: a
single outlier channel pushes every other channel's scaled values down fp16's window, where `lo` turns subnormal and the
representation error stops being relative (csrc/common.h).  Here the operands carry a real outlier 2^t above the bulk
(tests/pair_format_util.py: Operands) and
  * every kernel that writes planes reports exactly the documented scale, and its planes decode to the fp64 tensor within the
    documented representation bound, octave by octave of magnitude;
  * the three products stay within max(2 * the exact-split route's error, 2^-22) of the fp64 contraction up to t = 8, and beyond
    within twice what a CPU emulation of the documented format explains;
  * the scales hold at operand magnitudes 2^-60 .. 2^60 and for all-zero operands;
  * each producer of |max| words leaves the tensor's |max| bit for bit.
`pm_h2_clamp_events` stays put throughout: nothing here saturates — too LARGE a bound is what is probed."""
import ctypes as _ct
import functools

import numpy as np
import pytest
import torch

import pair_format_util as pf
from polyphemus_amd import _lib as _lib_mod
from polyphemus_amd import ops
from polyphemus_amd._lib import call, ptr, stream
from polyphemus_amd.synthetic import synthetic_batch
from test_kernels_gpu import DEV, _PmH2, _absmax_words, _pair_value, _planes_value, make_plan

pytestmark = pytest.mark.gpu
WS = pf.W_SCALE
SEED, LAYER = 5, 2                       # message dropout key


class _NormSums(_ct.Structure):          # PmNormSums (include/polyphemus_hip.h)
    _fields_ = [(k, _ct.c_void_p) for k in ("h", "mean", "var", "gamma", "beta")] + \
               [("eps", _ct.c_float), ("relu", _ct.c_int32), ("acc3", _ct.c_void_p), ("absmax_out", _ct.c_void_p)]


def _tile_kinds(plan):
    """(full 64-row tiles, partial tiles, 32-row halves, set of K-block counts) of the plan's GCL tile schedule"""
    tc = plan.field("trk_cnt")[:32].cpu().tolist()
    full = part = half = 0
    blocks = set()
    for grp, m0, rows in _lib_mod.gcl_tile_order(tc, True, plan.N):
        if grp < 0:
            continue
        M, cb = tc[grp], tc[8 + grp * 5: 13 + grp * 5]
        blocks.add(2 + int(m0 < cb[3] and m0 + rows > cb[1]) + int(m0 < cb[4] and m0 + rows > cb[2]))
        if rows == 32:
            half += 1
        elif m0 + 64 <= M:
            full += 1
        else:
            part += 1
    classes = [[cb_hi - cb_lo for cb_lo, cb_hi in zip(tc[8 + g * 5: 12 + g * 5], tc[9 + g * 5: 13 + g * 5])] for g in range(4)]
    return full, part, half, blocks, classes


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """sparse: the smallest batch with full and partial row tiles, tiles of different K-block counts and all sixteen node
    classes (track relation x {no, onset, onset + next, next} edges); dense: the bar route; split: more row tiles than CUs, so
    that some run as two 32-row halves (csrc/tile_order.h)"""
    if kind == "dense":
        cpu = synthetic_batch(2, 2, seed=17, dense=True)
    elif kind == "split":
        cpu = synthetic_batch(256, 2, p=0.25, seed=1235)
    else:
        cpu = synthetic_batch(16, 2, p=0.3, seed=29)
    b, plan = make_plan(cpu)
    full, part, half, blocks, classes = _tile_kinds(plan)
    if kind == "sparse":
        assert full > 0 and part > 0 and len(blocks) >= 2 and all(c > 0 for g in classes for c in g), (full, part, blocks, classes)
    if kind == "split":
        assert half > 0 and full > 0, (full, part, half)
    trel = plan.field("node_trel")[:plan.N].long().cpu()
    return cpu, plan, trel, pf.keep_blocks(cpu, 1).view(plan.N, 4)


def _keep(kind, d):
    return _graph(kind)[3].repeat_interleave(d, dim=1)


def _weight_planes(W, d, ws):
    """(kind-1, kind-0) fragment-major planes of W: exact bf16 triple, fp16 pair (plane 2 pre-set to a pattern)"""
    Wf3, Wft3 = ops.split_planes_frag(W, 1), ops.split_planes_frag(W, 0)
    Wf2, Wft2 = torch.full_like(Wf3, 77), torch.full_like(Wft3, 77)
    for kind, dst in ((1, Wf2), (0, Wft2)):
        call("pm_split_planes_frag_h2", ptr(W), 7 * d, d, kind, 1, 7 * d * d, 7 * d * d * 3, ws, ptr(dst), stream())
    return Wf3, Wft3, Wf2, Wft2


def _frag_values(Wf):
    """fragment-major planes [blocks][3][512] -> (planes 0, 1, 2) as flat int16"""
    v = Wf.reshape(-1, 3, 512)
    return v[:, 0].reshape(-1), v[:, 1].reshape(-1), v[:, 2].reshape(-1)


def _bf16(p):
    return (p.to(torch.int32) << 16).view(torch.float32).double()


def _planes3(n):
    """zeroed planes 0 / 1 (rows a kernel skips decode to 0), plane 2 pre-set: the pair format must leave it alone"""
    P = torch.zeros(3, n, dtype=torch.int16, device=DEV)
    P[2] = 77
    return P


def _run_layer(kind, o, p, ws=WS, route="fused"):
    """one GCL layer's three products on operands `o`, by the exact-split route ("3") and by the pair format ("2")"""
    cpu, plan, trel, _ = _graph(kind)
    N, d = plan.N, o.d
    dev = lambda t: t.to(DEV).contiguous()
    x, T, W, bias, du, hpre = dev(o.x), dev(o.T), dev(o.W), dev(o.bias), dev(o.du), dev(o.hpre)
    gamma, beta, mean, var = dev(o.gamma), dev(o.beta), dev(o.mean), dev(o.var)
    clamps0 = _lib_mod.h2_clamp_events()
    Wf3, Wft3, Wf2, Wft2 = _weight_planes(W, d, ws)
    mx, mt, mdu = _absmax_words(x), _absmax_words(T), _absmax_words(du)
    r = dict(N=N, d=d, Wf3=Wf3, Wf2=Wf2, Wft3=Wft3, Wft2=Wft2)
    # ---- forward
    P3, P2 = torch.zeros(3, N * 4 * d, dtype=torch.int16, device=DEV), _planes3(N * 4 * d)
    sA = torch.zeros(1, device=DEV)
    h2 = torch.empty(N, d, device=DEV)
    s3, s2 = (torch.zeros(8, 2, d, dtype=torch.float64, device=DEV) for _ in range(2))    # the norm's column sums: the measured epilogue
    hh = _PmH2(ptr(mx), ptr(mt), ptr(sA), ws, 0)
    if route == "bar":
        args = (ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, p, SEED, LAYER)
        call("pm_bar_aggregate_fwd", *args, ptr(P3), N * 4 * d, None, stream())
        call("pm_bar_aggregate_fwd", *args, ptr(P2), N * 4 * d, _ct.addressof(hh), stream())
        if d == 512:
            h3 = ops.gcl_forward_from_planes(P3, plan, d, Wf3, bias, col_stats=s3)
            call("pm_gcl_forward_from_planes_h2", ptr(P2), N * 4 * d, ptr(plan.buf), N, plan.E, plan.G, d, ptr(Wf2), ptr(bias), 1, ptr(h2),
                 ptr(s2), ptr(sA), ws, stream())
        else:
            h3 = h2 = None                                             # (the planes product of the bar route exists at d = 512 only)
    else:
        h3 = ops.gcl_forward_fused(x, T, plan, p, SEED, LAYER, Wf3, bias, col_stats=s3, planes=P3)
        call("pm_gcl_forward_fused_h2", ptr(x), ptr(T), ptr(plan.buf), N, plan.E, plan.G, d, p, SEED, LAYER, ptr(Wf2), ptr(bias), 1, ptr(h2),
             ptr(s2), ptr(P2), N * 4 * d, _ct.addressof(hh), stream())
    r.update(P3=P3, P2=P2, sa=float(sA), h3=h3, h2=h2)
    if h2 is None:
        r["clamps"] = _lib_mod.h2_clamp_events() - clamps0
        return r
    # ---- input gradient with the norm backward
    acc3 = ops.bn_bwd_sums(hpre, du, mean, var, gamma, beta)
    sdh = torch.zeros(1, device=DEV)
    dA2 = torch.full((N, 4 * d), float("nan"), device=DEV)
    D2 = _planes3(N * d)
    hb = _PmH2(ptr(mdu), None, ptr(sdh), ws, 0)
    if d <= 256:
        dA3, D3 = ops.gcl_input_grad_bn(hpre, du, mean, var, gamma, beta, acc3, plan, Wft3)
        nb = ops._BnBwd(ptr(hpre), ptr(du), ptr(mean), ptr(var), ptr(gamma), ptr(beta), ptr(acc3), None, None, None, 1e-5, 1, 0, 0)
        call("pm_gcl_input_grad_bn_h2", _ct.addressof(nb), ptr(D2), N * d, ptr(plan.buf), N, plan.E, plan.G, d, ptr(Wft2), 1, ptr(dA2),
             _ct.addressof(hb), stream())
    else:
        D3 = torch.zeros(3, N * d, dtype=torch.int16, device=DEV)
        call("pm_bn_bwd_fused", ptr(hpre), ptr(du), N, d, ptr(mean), ptr(var), 1e-5, ptr(gamma), ptr(beta), 1, None, None, None, None,
             ptr(acc3), ptr(D3), N * d, 1, stream())
        dA3 = ops.gcl_input_grad_fused(D3, plan, d, Wft3)
        call("pm_bn_bwd_fused_h2", ptr(hpre), ptr(du), N, d, ptr(mean), ptr(var), 1e-5, ptr(gamma), ptr(beta), 1, None, None, None,
             ptr(acc3), ptr(D2), N * d, 1, _ct.addressof(hb), stream())
        call("pm_gcl_input_grad_fused_h2", ptr(D2), N * d, ptr(plan.buf), N, plan.E, plan.G, d, ptr(Wft2), 1, ptr(dA2), ptr(sdh), ws,
             stream())
    r.update(D3=D3, D2=D2, sdh=float(sdh), dA3=dA3, dA2=dA2)
    # ---- weight gradient (+=) from each route's two plane sets
    mag = float(o.x.abs().median() * o.du.abs().median()) or 1.0
    base = dev(torch.randn(7 * d, d, generator=torch.Generator().manual_seed(3)) * mag)
    dW3, dW2 = base.clone(), base.clone()
    ops.gcl_weight_grad_fused(P3, D3, plan, d, dW3)
    call("pm_gcl_weight_grad_fused_h2", ptr(P2), N * 4 * d, ptr(D2), N * d, ptr(plan.buf), N, plan.E, plan.G, d, 1, ptr(dW2), ptr(sA),
         ptr(sdh), stream())
    r.update(base=base, dW3=dW3, dW2=dW2, clamps=_lib_mod.h2_clamp_events() - clamps0)
    return r


def _product_errors(kind, o, r):
    """{product: (err_pair, err_triple, err_model)}: relative L2 against the fp64 contraction (CPU) of the fp32 operands — the
    exact-split route's planes decode to them exactly; the model is the CPU emulation run with the scales the kernels reported"""
    cpu, plan, trel, _ = _graph(kind)
    N, d = r["N"], r["d"]
    A32 = _planes_value(r["P3"]).float().view(N, 4 * d).cpu()
    dh32 = _planes_value(r["D3"]).float().view(N, d).cpu()
    assert torch.equal(A32[:, 3 * d:], o.x)                            # the split is exact: the self block is x
    masks = pf.compared(o, _keep(kind, d))
    ref = pf.plain_products(o, A32, dh32, trel)
    model = pf.model_products(o, A32, dh32, trel, r["sa"], r["sdh"], WS)
    base, bias = r["base"].double().cpu(), o.bias.double()
    got = {}
    for tag in ("2", "3"):
        got[tag] = {"forward": r["h" + tag].double().cpu() - bias, "input_grad": r["dA" + tag].double().cpu(),
                    "weight_grad": r["dW" + tag].double().cpu() - base}
        for k, v in got[tag].items():
            assert bool(torch.isfinite(v if masks[k] is None else v[masks[k]]).all()), (tag, k)
    # (h - bias and dW - base round once more in fp64: 2^-53 relative, nothing next to 2^-24)
    e2, e3, em = pf.errors(got["2"], ref, masks), pf.errors(got["3"], ref, masks), pf.errors(model, ref, masks)
    return {k: (e2[k], e3[k], em[k]) for k in ref}


def _check_products(kind, o, r, tag):
    errs = _product_errors(kind, o, r)
    bad = []
    for k, (e2, e3, em) in errs.items():
        lim = pf.condition(o.t, o.heavy, e2, e3, em)
        print(f"PAIRFMT {tag} {k}: err_pair {e2:.2e} err_triple {e3:.2e} err_model {em:.2e} bound {lim:.2e}")
        if not e2 <= lim:
            bad.append((k, e2, e3, em, lim))
    assert not bad, bad
    assert r["clamps"] == 0
    return errs


# ---------------------------------------------------------------------------------------------- 3. the products
CASES = [("sparse", d, p, t) for d, p in ((128, 0.0), (256, 0.1)) for t in (0, 4, 8, 12, 16)] + \
        [("sparse", 512, 0.1, t) for t in (0, 8, 12)] + [("dense", 512, 0.1, t) for t in (0, 8, 12)] + [("split", 128, 0.1, 8)]


@pytest.mark.parametrize("kind,d,p,t", CASES)
def test_products_across_dynamic_range(kind, d, p, t):
    """One channel of x and one of du sit 2^t above the bulk (the weight's matching rows / column are zero, so no compared
    output depends on them, yet they set the |max| words and with them the scales).  t <= 8: err_pair <= max(2 err_triple,
    2^-22) — a second form of the same kernel; t >= 12: err_pair <= 2 (err_model + err_triple) — the loss is the one the
    documented representation explains (a conversion or matrix core flushing fp16 subnormals would miss it a hundredfold).
    dense: pm_bar_aggregate_fwd + pm_gcl_forward_from_planes_h2."""
    cpu, plan, trel, _ = _graph(kind)
    o = pf.Operands(plan.N, d, t=t)
    r = _run_layer(kind, o, p, route="bar" if kind == "dense" else "fused")
    assert r["sa"] == o.agg_scale(p) and r["sdh"] == o.dh_scale(), (r["sa"], o.agg_scale(p), r["sdh"], o.dh_scale())
    _check_products(kind, o, r, f"{kind} d={d} t=2^{t}")


def test_products_on_heavy_tailed_operands():
    """x and du = randn * 2^(3 randn) elementwise, nothing excluded: |max| / median >= 2^8; held to the model condition."""
    cpu, plan, trel, _ = _graph("sparse")
    o = pf.Operands(plan.N, 128, heavy=True)
    for v in (o.x, o.du):
        assert float(v.abs().max() / v.abs().median()) >= 2.0 ** 8
    r = _run_layer("sparse", o, 0.1)
    assert r["sa"] == o.agg_scale(0.1) and r["sdh"] == o.dh_scale()
    _check_products("sparse", o, r, "sparse d=128 heavy tails")


# ---------------------------------------------------------------------------------------------- 2. scales and planes
def _check_planes(name, pair, triple, ref64, s):
    bad = []
    for top, err, lim in pf.octave_errors(pair, triple, ref64, s):
        print(f"PAIRFMT planes {name}: |v s| < 2^{int(np.log2(top))}: max err {err:.3e} allowed {lim:.3e}")
        if not err <= lim:
            bad.append((top, err, lim))
    assert not bad, (name, bad)


@pytest.mark.parametrize("kind,d,p,route", [("sparse", 128, 0.0, "fused"), ("sparse", 256, 0.1, "fused"), ("sparse", 512, 0.1, "fused"),
                                            ("dense", 128, 0.1, "bar")])
def test_reported_scales_and_plane_representation(kind, d, p, route):
    """Every producer of pair-format planes at t = 12 (bulk in the subnormal-lo half of the bound, outlier channel in the normal
    half): pm_gcl_forward_fused_h2 (d = 512: wide.hip), pm_bar_aggregate_fwd, pm_gcl_input_grad_bn_h2 (d <= 256),
    pm_bn_bwd_fused_h2 (d = 512), pm_split_planes_frag_h2.  scale_out is the documented formula exactly; the planes decode to the
    fp64 tensor within the representation bound per octave of |v s| (+ twice the exact-split route's own distance from fp64: the
    fp32 evaluation both share); plane 2 is left alone; nothing saturates."""
    cpu, plan, trel, _ = _graph(kind)
    N = plan.N
    o = pf.Operands(N, d, t=12)
    assert pf.clear_of_pow2(o.dh_bound())                              # rsqrtf's rounding cannot move the binade
    r = _run_layer(kind, o, p, route=route)
    assert r["clamps"] == 0
    # ---- aggregates: |A'| <= |x|max * max(1, |T|max / (1 - p))
    assert r["sa"] == o.agg_scale(p), (r["sa"], o.agg_scale(p))
    A64 = pf.aggregate64(o.x.double(), o.T.double(), cpu, trel, p, SEED, LAYER)
    _check_planes("A'", _pair_value(r["P2"], r["sa"]).view(N, 4 * d), _planes_value(r["P3"]).view(N, 4 * d), A64, r["sa"])
    assert bool((r["P2"][2] == 77).all())
    # ---- weights: W * w_scale itself is the reference (the fragment order is that of the exact-split planes)
    for f3, f2 in ((r["Wf3"], r["Wf2"]), (r["Wft3"], r["Wft2"])):
        a, b, c = _frag_values(f3)
        Wfrag = _bf16(a) + _bf16(b) + _bf16(c)
        assert torch.equal(Wfrag.sort().values, o.W.double().flatten().sort().values.to(DEV))
        h, l, third = _frag_values(f2)
        pair = (h.view(torch.float16).double() + l.view(torch.float16).double()) / WS
        _check_planes("W", pair, Wfrag, Wfrag, WS)
        assert bool((third == 77).all())
    if route == "bar":
        return
    # ---- dh: |dh| <= max_c |gamma_c rstd_c| * |du|max * 16
    assert r["sdh"] == o.dh_scale(), (r["sdh"], o.dh_scale())
    dh64 = pf.bn_bwd64(o.hpre, o.du, o.mean, o.var, o.gamma, o.beta)
    _check_planes("dh", _pair_value(r["D2"], r["sdh"]).view(N, d), _planes_value(r["D3"]).view(N, d), dh64, r["sdh"])
    assert bool((r["D2"][2] == 77).all())


# ---------------------------------------------------------------------------------------------- 4. scale edges
@pytest.mark.parametrize("xs,gs", [(2.0 ** -60, 1.0), (2.0 ** 60, 1.0), (1.0, 2.0 ** -60), (1.0, 2.0 ** 60)])
def test_products_at_extreme_operand_magnitudes(xs, gs):
    cpu, plan, trel, _ = _graph("sparse")
    o = pf.Operands(plan.N, 128, t=0, xs=xs, gs=gs)
    r = _run_layer("sparse", o, 0.0)
    assert r["sa"] == o.agg_scale(0.0) and r["sdh"] == o.dh_scale(), (r["sa"], o.agg_scale(0.0), r["sdh"], o.dh_scale())
    _check_products("sparse", o, r, f"sparse d=128 xs=2^{int(np.log2(xs))} gs=2^{int(np.log2(gs))}")


def test_all_zero_operands():
    """x = 0: scale 1, zero planes, h == bias exactly.  du = 0: zero dh planes, dA' and the dW increment exactly zero."""
    cpu, plan, trel, _ = _graph("sparse")
    N, d = plan.N, 128
    o = pf.Operands(N, d, t=0)
    o.x.zero_()
    o.du.zero_()
    r = _run_layer("sparse", o, 0.1)
    assert r["sa"] == 1.0 and r["sdh"] == 1.0
    assert int(r["P2"][:2].abs().max()) == 0 and int(r["D2"][:2].abs().max()) == 0
    assert bool((r["P2"][2] == 77).all()) and bool((r["D2"][2] == 77).all())
    assert torch.equal(r["h2"], o.bias.to(DEV).expand(N, d))
    keep = _keep("sparse", d).to(DEV)
    assert bool(torch.isfinite(r["dA2"][keep]).all()) and float(r["dA2"][keep].abs().max()) == 0.0
    assert torch.equal(r["dW2"], r["base"])
    assert r["clamps"] == 0


# ---------------------------------------------------------------------------------------------- 5. the |max| producers
ROWS_COLS = [(O, C) for O in (1, 63, 257, 1000) for C in (128, 512)]


def _spots(O, C):
    """where the extreme element goes: row 0, the last row, the last column"""
    return [(0, C // 3), (O - 1, C // 2), (O // 2, C - 1)]


def _words(fill=0.0):
    return torch.full((64,), fill, dtype=torch.float32, device=DEV).view(torch.int32)


def _check_words(run, tensor_absmax):
    """`run(words)` launches the producer; the maximum of the 64 words is the tensor's |max| bit for bit from zeroed words and from
    words at a smaller earlier maximum (none of which is lowered); words at a larger earlier maximum keep it"""
    for fill in (0.0, 0.5 ** 20):
        w = _words(fill)
        run(w)
        wf = w.view(torch.float32)
        assert float(wf.max()) == tensor_absmax(), (fill, float(wf.max()), tensor_absmax())
        assert float(wf.min()) >= fill
    big = _words(2.0 ** 40)
    run(big)
    assert torch.equal(big, _words(2.0 ** 40))


@pytest.mark.parametrize("O,C", ROWS_COLS)
def test_absmax_of_bn_apply(O, C):
    """pm_bn_apply_fused_absmax: max |y| of the y it wrote (BatchNorm + residual, no ReLU: the extreme is negative)."""
    g = torch.Generator().manual_seed(O * 7 + C)
    x = torch.randn(O, C, generator=g).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    sums = torch.zeros(8, 2, C, dtype=torch.float64, device=DEV)
    sums[0, 0], sums[0, 1] = x.double().sum(0), (x.double() ** 2).sum(0)
    for (r, c) in _spots(O, C):
        res = torch.randn(O, C, generator=g).to(DEV)
        res[r, c] = -1000.0
        y = torch.empty(O, C, device=DEV)
        mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)

        def run(w):
            call("pm_bn_apply_fused_absmax", ptr(x), O, C, ptr(sums), 1e-5, ptr(gamma), ptr(beta), ptr(res), 0, ptr(y), ptr(mean), ptr(var),
                 None, None, 0.1, ptr(w), stream())
        _check_words(run, lambda: float(y.abs().max()))
        assert int(y.abs().argmax()) == r * C + c and float(y[r, c]) < -900.0


@pytest.mark.parametrize("O,C", ROWS_COLS)
def test_absmax_of_bn_backward_sums(O, C):
    """pm_bn_bwd_sums_absmax tracks the raw dy it reads, not the ReLU-masked du (norm.hip k_colreduce_rows_bwd_atomic): a bound
    for |du|, as the dh scale needs.  Its column sums are those of pm_bn_bwd_sums."""
    g = torch.Generator().manual_seed(O * 11 + C)
    x = (torch.randn(O, C, generator=g) * 1.5 + 0.3).to(DEV)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.randn(C, generator=g) * 0.2).to(DEV)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    for (r, c) in _spots(O, C):
        dy = torch.randn(O, C, generator=g).to(DEV)
        dy[r, c] = -1000.0
        acc = []

        def run(w):
            acc3 = torch.zeros(8, 3, C, dtype=torch.float64, device=DEV)
            call("pm_bn_bwd_sums_absmax", ptr(x), ptr(dy), O, C, ptr(mean), ptr(var), 1e-5, ptr(gamma), ptr(beta), 1, ptr(acc3), ptr(w),
                 stream())
            acc.append(acc3.sum(0))
        _check_words(run, lambda: float(dy.abs().max()))
        assert float(dy.abs().max()) == 1000.0
        on = (x - mean) * torch.rsqrt(var + 1e-5) * gamma + beta > 0
        assert 1000.0 >= float(torch.where(on, dy, torch.zeros_like(dy)).abs().max())
        want = ops.bn_bwd_sums(x, dy, mean, var, gamma, beta).sum(0)
        assert float((acc[0] - want).abs().max()) <= 1e-9 * float(want.abs().max())


@pytest.mark.parametrize("O,C", ROWS_COLS)
def test_absmax_of_chord_sum(O, C):
    """pm_chord_sum_fwd_absmax: max of the x0 it wrote (x0 = relu(...) >= 0: the extreme is a positive table entry that only
    the chosen node's first token reaches)."""
    g = torch.Generator().manual_seed(O * 13 + C)
    N, d, S = O, C, 2
    tok = torch.zeros(N, 16, 2, dtype=torch.int32)
    tok[:, :, 0] = torch.randint(0, 129, (N, 16), generator=g, dtype=torch.int32)
    tok[:, :, 1] = torch.randint(0, 99, (N, 16), generator=g, dtype=torch.int32)
    drum = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
    cvec = (torch.randn(2, d, generator=g) * 0.1).to(DEV)
    for (r, c) in _spots(N, d):
        t = tok.clone()
        t[r, 1, 0] = 130                                               # the first kept slot's pitch token of node r alone
        PT = torch.randn(2, S, 2, 131, d, generator=g) * 0.5
        PT[:, 0, 0, 130] = 0.0
        PT[1 - int(drum[r]), 0, 0, 130, c] = 1000.0
        td, PTd, dd = t.to(DEV), PT.to(DEV), drum.to(DEV)
        x0 = torch.empty(N, d, device=DEV)

        def run(w):
            call("pm_chord_sum_fwd_absmax", ptr(PTd), ptr(cvec), ptr(td), ptr(dd), N, d, S, ptr(x0), ptr(w), stream())
        _check_words(run, lambda: float(x0.max()))
        assert int(x0.argmax()) == r * d + c and float(x0[r, c]) > 900.0
        grp = 1 - dd.long()
        pit, dur = td[:, 1:S + 1, 0].long(), td[:, 1:S + 1, 1].long()
        ref = cvec.double()[grp]
        for s in range(S):
            ref = ref + PTd.double()[grp, s, 0, pit[:, s]] + PTd.double()[grp, s, 1, dur[:, s]]
        assert float((x0.double() - torch.relu(ref)).abs().max()) <= 1e-5 * 1000.0


@pytest.mark.parametrize("d", [128, 256])
def test_absmax_of_segreduce_backward(d):
    """PmNormSums.absmax_out of pm_segreduce_bwd_norm: max |dx| of the dx it wrote (the extreme enters through the residual)."""
    cpu, plan, trel, _ = _graph("sparse")
    N = plan.N
    g = torch.Generator().manual_seed(d)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    x, T, dA, hpre = rn(N, d), rn(32, d) * 0.5, rn(N, 4 * d), rn(N, d) * 1.5 + 0.3
    gamma, beta = torch.rand(d, generator=g).to(DEV) + 0.5, rn(d) * 0.2
    mean, var = hpre.mean(0), hpre.var(0, unbiased=False)
    for (r, c) in _spots(N, d):
        dres = rn(N, d)
        dres[r, c] = -1.0e4
        dx = torch.empty(N, d, device=DEV)

        def run(w):
            acc3 = torch.zeros(8, 3, d, dtype=torch.float64, device=DEV)
            dT = torch.zeros(32, d, device=DEV)
            nn = _NormSums(ptr(hpre), ptr(mean), ptr(var), ptr(gamma), ptr(beta), 1e-5, 1, ptr(acc3), ptr(w))
            call("pm_segreduce_bwd_norm", ptr(x), ptr(T), ptr(dA), ptr(dres), ptr(plan.buf), N, plan.E, plan.G, d, 0.1, 9, 4, 1, ptr(dx),
                 ptr(dT), _ct.addressof(nn), stream())
        _check_words(run, lambda: float(dx.abs().max()))
        assert int(dx.abs().argmax()) == r * d + c and float(dx[r, c]) < -9.0e3
