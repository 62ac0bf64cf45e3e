"""Every matrix-core product of the library, bit for bit, on operands on which nothing rounds (tests/exact_util.py).

Every assertion on a product is `torch.equal(out.double(), model)`: the model is the fp64 sum of the six kept bf16 products
(`kept6`; three fp16 pair products, `kept3`), or the fp64 product itself for the fp32 tiles on the two-term lattice.  Each case
runs at nnz = 1 and 6 non-zeros per slice of the sparse operand, once plain and once graded by exact powers of two per output
row and column.  Where a bias is added the row scales stay in 2^0 .. 2^16 (exact_util.pow2_scales says why); accumulate
bases carry row x column scale and take the full 2^-20 .. 2^20.

The sparse operand is the one that indexes the output row; where that one has too few rows to put a non-zero on every k
(fewer than ceil(K / nnz)) and the other operand has enough columns, the other one is the sparse one (the bound on
sum |x||y| is symmetric); where neither can, the case runs uncovered at nnz = 1 and its nnz = 6 twin covers every k.

Entry points that cannot be driven with hand-made planes: `pm_gcl_forward_from_planes` exists at d = 512 only (at 128 / 256
the forward builds its aggregate in the kernel), `pm_gcl_input_grad_fused_h2` at d = 512 only (at 256 the norm backward
builds dh in the kernel).  The existing tests tie those to the entries below."""
import ctypes

import pytest
import torch

import exact_util as X
from polyphemus_amd import ops
from polyphemus_amd import _lib as _lib_mod
from polyphemus_amd._lib import PROF_NCLASS, call, lib, ptr, stream
from polyphemus_amd.synthetic import synthetic_batch
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
CASES = [(nnz, graded) for nnz in X.NNZ for graded in (False, True)]
case_ids = lambda c: f"nnz{c[0]}-{'graded' if c[1] else 'plain'}"
each_case = pytest.mark.parametrize("case", CASES, ids=case_ids)


def _gen(*key):
    return torch.Generator(device=DEV).manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 23)


def _operands(M, N, K, nnz, g, lattice=X.lattice3, side=None):
    """(row operand [M, K], column operand [K, N]) on the lattice, one of them sparse along K (see the module docstring)"""
    need = -(-K // nnz)
    if side is None:
        side = "row" if M >= need or N < need else "col"
    Ar, Bc = lattice((M, K), g), lattice((K, N), g)
    if side == "row":
        Ar = X.sparsify(Ar, 1, nnz, cover=M >= need)
    else:
        Bc = X.sparsify(Bc, 0, nnz, cover=N >= need)
    return Ar, Bc


def _scales(M, N, graded, g, bias=False):
    """(row scales [M], column scales [N], their outer product [M, N]); all ones when not graded"""
    if not graded:
        return torch.ones(M, dtype=torch.float64, device=DEV), torch.ones(N, dtype=torch.float64, device=DEV), None
    r = X.pow2_scales(M, g, 16, 0) if bias else X.pow2_scales(M, g)
    c = X.pow2_scales(N, g)
    return r, c, r[:, None] * c[None, :]


def _fp32(model):
    """the model as fp32 words; it must be one"""
    assert torch.equal(model.float().double(), model)
    return model


def _padded(x, ld, fill=NAN):
    """x [rows, cols] inside a [rows, ld] buffer filled with NaN; returns the buffer"""
    buf = torch.full((x.shape[0], ld), fill, device=DEV)
    buf[:, :x.shape[1]] = x
    return buf


def _launch_classes(fn):
    """launch counts per profiler class of the calls in fn (GEMM class = 3 * configuration id + layout)"""
    L = lib()
    try:
        L.pm_prof_configure(-1, 1)
        L.pm_prof_begin(64)
        fn()
        torch.cuda.synchronize()
        ms, work, cnt = (ctypes.c_double * PROF_NCLASS)(), (ctypes.c_double * PROF_NCLASS)(), (ctypes.c_int64 * PROF_NCLASS)()
        assert L.pm_prof_end(ctypes.cast(ms, ctypes.c_void_p), ctypes.cast(work, ctypes.c_void_p),
                             ctypes.cast(cnt, ctypes.c_void_p)) == 0
    finally:
        L.pm_prof_configure(-1, 1)
    return list(cnt)


# ------------------------------------------------------------------ ops.gemm / ops.gemm_desc: every row of GEMM_CFGS
def _gemm_case(cfg, M, N, K, ta, tb, nnz, graded, lda=0, ldb=0, cpad=0):
    """One product on tile configuration `cfg`: 0 / 2 fp32 tiles (two-term lattice, model = the fp64 product), 4 / 5 / 7 the
    in-kernel split (pinned by pm_gemm_force_config), 8 / 9 pre-split planes (9: B also as fragment-major planes).  NN / NT
    with bias + ReLU (9: bias + column sums); TN accumulating (split_k = 0) with the bias gradient (`a_colsum`) where the
    entry takes one.  `lda`, `ldb`: NaN-filled row pitches; `cpad`: columns of C beyond N that must keep their 7.0.  The
    launch is counted by the profiler: the tile under test must be the one that ran."""
    fp32, planes = cfg in (0, 2), cfg in (8, 9)
    g = _gen(cfg, M, N, K, nnz, graded)
    Ar, Bc = _operands(M, N, K, nnz, g, X.lattice2 if fp32 else X.lattice3, side="row" if ta else None)
    r, c, scale = _scales(M, N, graded, g, bias=not ta)
    Ar, Bc = X.scale_by(Ar, r, 0), X.scale_by(Bc, c, 1)
    model = X.exact_mm(Ar, Bc, scale) if fp32 else X.kept6(Ar, Bc, scale)
    A = Ar.t().contiguous() if ta else Ar
    B = Bc.t().contiguous() if tb else Bc
    lda, ldb = lda or A.shape[1], ldb or B.shape[1]
    A, B = _padded(A, lda), _padded(B, ldb)
    ldc = N + cpad
    lay = 2 if ta else (1 if tb else 0)
    kw = dict(transA=ta, transB=tb)
    if planes:
        kw.update(planes=True, a_plane_stride=A.numel(), b_plane_stride=B.numel())
        if cfg == 9:
            kw.update(b_frag=ops.split_planes_frag(B, 0 if tb else 1))
        A_, B_ = ops.split_planes(A), ops.split_planes(B)
    else:
        A_, B_ = A, B
    if not ta:
        bias = X.scale_by(X.base_lattice((N,), g), c, 0)
        relu = cfg != 9                                              # (config 9 with column statistics instead, as the GCL forward)
        want = _fp32(torch.relu(model + bias.double()) if relu else model + bias.double())
        out = torch.full((M, ldc), 7.0, device=DEV)
        stats = torch.zeros(8, 2, N, dtype=torch.float64, device=DEV) if cfg == 9 else None
        if stats is not None:
            kw.update(col_stats=stats)
        run = lambda: ops.gemm_desc(A_, B_, out, M, N, K, lda, ldb, ldc, bias=bias, relu=relu, **kw)
    else:
        base = X.base_lattice((M, N), g)
        base = base if scale is None else (base.double() * scale).float()
        want = _fp32(base.double() + model)
        out = torch.full((M, ldc), 7.0, device=DEV)
        out[:, :N] = base
        kw.update(accum=True, split_k=0)
        if not planes:
            db0 = X.scale_by(X.base_lattice((M,), g), r, 0)
            db = db0.clone()
            kw.update(a_colsum=db)
        run = lambda: ops.gemm_desc(A_, B_, out, M, N, K, lda, ldb, ldc, **kw)
    try:
        if not planes:
            assert lib().pm_gemm_force_config(cfg) == 0
        cnt = _launch_classes(run)
    finally:
        lib().pm_gemm_force_config(-1)
    assert cnt[3 * cfg + lay] == 1, [(k, n) for k, n in enumerate(cnt) if n]       # the tile under test is the one that ran
    assert torch.equal(out[:, :N].double(), want)
    assert bool((out[:, N:] == 7.0).all())
    if ta and not planes:
        assert torch.equal(db.double(), _fp32(db0.double() + Ar.double().sum(1)))
    if not ta and cfg == 9:
        assert rel_err(stats.sum(0)[0], out[:, :N].double().sum(0)) < 1e-9


# (the K tail of the 16- and 32-wide k-tiles, M / N tails of 64- and 128-wide tiles, more than one tile each way)
GEMM_SHAPES = [(130, 132, 36, False, True), (515, 260, 72, False, False), (260, 68, 1028, True, False)]
# planes: 16-byte chunks of 8 bf16 along each contiguous extent, so those extents are multiples of 8 (64x64x32 tiles)
PLANES_SHAPES = [(130, 132, 40, False, True), (515, 264, 72, False, False), (264, 72, 1028, True, False)]


@each_case
@pytest.mark.parametrize("cfg,M,N,K,ta,tb", [(cfg, *s) for cfg in (0, 2, 4, 5, 7) for s in GEMM_SHAPES if cfg in (0, 2) or s[3] == (cfg == 5)])
def test_gemm_tiles(cfg, M, N, K, ta, tb, case):
    _gemm_case(cfg, M, N, K, ta, tb, *case)


@each_case
@pytest.mark.parametrize("cfg", [0, 2])
def test_gemm_fp32_tiles_ragged_extents_in_aligned_rows(cfg, case):
    """(70, 131, 130) NN with row pitches of 132: the float4 that straddles the end of an extent reads NaN"""
    _gemm_case(cfg, 70, 131, 130, False, False, *case, lda=132, ldb=132, cpad=3)


@each_case
@pytest.mark.parametrize("M,N,K,ta,tb", PLANES_SHAPES)
def test_gemm_planes_tile(M, N, K, ta, tb, case):
    _gemm_case(8, M, N, K, ta, tb, *case)


@each_case
@pytest.mark.parametrize("M,N,K,tb", [(64, 128, 32, True), (300, 128, 256, False), (130, 384, 96, False)])
def test_gemm_planes_b_direct_tile(M, N, K, tb, case):
    """config 9: 64x128x32 (NT) and 64x128x64 (NN) tiles, B from fragment-major planes; K = 256 = 4 d of the forward"""
    _gemm_case(9, M, N, K, False, tb, *case)


@each_case
def test_gemm_rowmap_form(case):
    """the content-decoder routing of test_gemm_strided_views_and_rowmap: rows = (node, slot) pairs of a node list with a
    device-side count, strided A (the unused half of each row is NaN) and C (untouched rows and columns stay zero)"""
    nnz, graded = case
    Nn, d, S = 50, 64, 15
    g = _gen(Nn, d, nnz, graded)
    Ar, Bc = _operands(Nn * S, 131, d // 2, nnz, g, X.lattice2)
    r, c, scale = _scales(Nn * S, 131, graded, g)
    Ar, Bc = X.scale_by(Ar, r, 0), X.scale_by(Bc, c, 1)
    H = _padded(Ar, d)
    Wp = Bc.t().contiguous()
    logits = torch.zeros(Nn, S, 230, device=DEV)
    nodes = torch.tensor([3, 7, 8, 20, 41, 49], dtype=torch.int32, device=DEV)
    cnt = torch.tensor([5], dtype=torch.int32, device=DEV)               # only the first 5 entries are live
    ops.gemm(H, Wp, logits, nodes.numel() * S, 131, d // 2, d, d // 2, 230, transB=True, rowmap=nodes, rows_per_entry=S,
             dyn_entries=cnt)
    want = torch.zeros(Nn, S, 230, dtype=torch.float64, device=DEV)
    sel = nodes[:5].long()
    want[sel, :, :131] = X.exact_mm(Ar, Bc, scale).view(Nn, S, 131)[sel]
    assert torch.equal(logits.double(), want)


@each_case
@pytest.mark.parametrize("planes", [True, "bfrag"])
def test_gemm_grouped_stacked_partitioned(planes, case):
    """The three contractions of the compact GCL through the descriptor (test_gemm_grouped_stacked_compact_gcl at Nn = 333,
    d = 128, partitioned row lists): forward with bias, input gradient, accumulating weight gradient."""
    nnz, graded = case
    Nn, d = 333, 128
    dd = d * d
    g = _gen(Nn, d, nnz, graded, planes == "bfrag")
    trel = torch.randint(0, 4, (Nn,), generator=g, device=DEV)
    trel[: Nn // 3] = 2                                           # uneven groups
    lists = torch.full((4, Nn), -7, dtype=torch.int32, device=DEV)   # entries past the live count are never read
    cnt = torch.zeros(8, dtype=torch.int32, device=DEV)
    for t in range(4):
        rows = torch.nonzero(trel == t).flatten().to(torch.int32)
        lists[t, : rows.numel()] = rows.flip(0)
        cnt[t] = rows.numel()
    grp = dict(rowmap=lists, rows_per_entry=1, dyn_entries=cnt, n_groups=4, map_group_stride=Nn, dyn_group_stride=1,
               partition=True, planes=True)
    wn = lambda W, t: torch.cat([W[t * d:(t + 1) * d], W[4 * d:]])    # [4d, d] of relation t
    # forward: h = A [W_t; W_4; W_5; root] + bias; rows of A sparse
    A = X.sparsify(X.lattice3((Nn, 4 * d), g), 1, nnz, cover=False)
    W = X.lattice3((7 * d, d), g)
    r, c, scale = _scales(Nn, d, graded, g, bias=True)
    A, W = X.scale_by(A, r, 0), X.scale_by(W, c, 1)
    bias = X.scale_by(X.base_lattice((d,), g), c, 0)
    fn = dict(b_frag=ops.split_planes_frag(W, 1)) if planes == "bfrag" else {}
    h = torch.full((Nn, d), NAN, device=DEV)
    ops.gemm_desc(ops.split_planes(A), ops.split_planes(W), h, Nn, d, 4 * d, 4 * d, d, d, bias=bias, b_group_stride=dd,
                  b_split_rows=d, b_shared_off=3 * dd, a_plane_stride=A.numel(), b_plane_stride=W.numel(), **grp, **fn)
    want = torch.empty(Nn, d, dtype=torch.float64, device=DEV)
    for t in range(4):
        m = trel == t
        want[m] = X.kept6(A[m], wn(W, t), None if scale is None else scale[m]) + bias.double()
    assert torch.equal(h.double(), _fp32(want))
    # input gradient: dA = dh [W_t; W_4; W_5; root]^T; rows of dh sparse, the rows of W carry the column scales
    dh = X.sparsify(X.lattice3((Nn, d), g), 1, nnz, cover=True)
    W = X.lattice3((7 * d, d), g)
    r, c, _ = _scales(Nn, 4 * d, graded, g)
    c7 = torch.cat([c[:d]] * 4 + [c[d:]])
    dh, W = X.scale_by(dh, r, 0), X.scale_by(W, c7, 0)
    ft = dict(b_frag=ops.split_planes_frag(W, 0)) if planes == "bfrag" else {}
    dA = torch.full((Nn, 4 * d), NAN, device=DEV)
    ops.gemm_desc(ops.split_planes(dh), ops.split_planes(W), dA, Nn, 4 * d, d, d, d, 4 * d, transB=True, b_group_stride=dd,
                  b_split_rows=d, b_shared_off=3 * dd, a_plane_stride=dh.numel(), b_plane_stride=W.numel(), **grp, **ft)
    want = torch.empty(Nn, 4 * d, dtype=torch.float64, device=DEV)
    for t in range(4):
        m = trel == t
        want[m] = X.kept6(dh[m], wn(W, t).t().contiguous(), (r[m, None] * c[None, :]) if graded else None)
    assert torch.equal(dA.double(), want)
    # weight gradient: dW += A^T dh per group (track rows) / over all rows (shared rows); columns of A sparse
    A = X.sparsify(X.lattice3((Nn, 4 * d), g), 0, nnz, cover=True)
    dh = X.lattice3((Nn, d), g)
    r, c, scale = _scales(4 * d, d, graded, g)
    A, dh = X.scale_by(A, r, 1), X.scale_by(dh, c, 1)
    r7 = torch.cat([r[:d]] * 4 + [r[d:]])
    base = (X.base_lattice((7 * d, d), g).double() * r7[:, None] * c[None, :]).float()
    dW = base.clone()
    ops.gemm_desc(ops.split_planes(A), ops.split_planes(dh), dW, 4 * d, d, Nn, 4 * d, d, d, transA=True, accum=True,
                  split_k=0, c_group_stride=dd, c_split_rows=d, c_shared_off=3 * dd, a_plane_stride=A.numel(),
                  b_plane_stride=dh.numel(), **grp)
    assert torch.equal(dW.double(), _fp32(base.double() + _gcl_dw_model(A, dh, trel, d, r, c, graded)))


def _gcl_dw_model(A, dh, trel, d, r, c, graded, kept=X.kept6):
    """[7d, d]: A[:, :d]^T dh over the rows of each track relation, A[:, d:]^T dh over all rows (r: scales of A's columns)"""
    out = torch.zeros(7 * d, d, dtype=torch.float64, device=A.device)
    sc = (lambda lo, hi: r[lo:hi, None] * c[None, :]) if graded else (lambda lo, hi: None)
    for t in range(4):
        m = trel == t
        if bool(m.any()):
            out[t * d:(t + 1) * d] = kept(A[m, :d].t().contiguous(), dh[m], sc(0, d))
    out[4 * d:] = kept(A[:, d:].t().contiguous(), dh, sc(d, 4 * d))
    return out


# ------------------------------------------------------------------ the row-tile products of linear.hip / wide.hip
@each_case
@pytest.mark.parametrize("K,Nout,N,kind", [(128, 384, 77, 0), (128, 256, 64, 1), (512, 512, 64, 0)])
def test_rows_times_weight(K, Nout, N, kind, case):
    """`pm_rows_times_weight`, both weight orientations (kind 0 with bias) and the 512-wide route of wide.hip; strided x
    (NaN beyond K) and y (7.0 beyond Nout)"""
    nnz, graded = case
    g = _gen(K, Nout, N, kind, nnz, graded)
    ldx, ldc = K + 8, Nout + 4
    Xr, Wc = _operands(N, Nout, K, nnz, g)
    r, c, scale = _scales(N, Nout, graded, g, bias=kind == 0)
    Xr, Wc = X.scale_by(Xr, r, 0), X.scale_by(Wc, c, 1)
    want = X.kept6(Xr, Wc, scale)
    bias = None
    if kind == 0:
        W, tiles = Wc.t().contiguous(), 0                              # [Nout, K]
        bias = X.scale_by(X.base_lattice((Nout,), g), c, 0)
        want = _fp32(want + bias.double())
    else:
        ldw = Nout + 3 * K                                             # the product uses the first Nout columns of W [K, ldw]
        W = X.lattice3((K, ldw), g)
        W[:, :Nout] = Wc
        tiles = ldw // 32
    Wf = ops.split_planes_frag(W, kind)
    C = torch.full((N, ldc), 7.0, device=DEV)
    call("pm_rows_times_weight", ptr(_padded(Xr, ldx)), ldx, N, K, ptr(Wf), kind, tiles, Nout, ptr(bias), ptr(C), ldc, stream())
    assert torch.equal(C[:, :Nout].double(), want)
    assert bool((C[:, Nout:] == 7.0).all())


@each_case
@pytest.mark.parametrize("K,Nout,N,kind", [(384, 128, 77, 0), (128, 128, 64, 1), (128, 512, 64, 1), (1536, 512, 260, 1)])
def test_rows_times_weight_longk(K, Nout, N, kind, case):
    """`pm_rows_times_weight_longk`, both orientations and the 512-wide route of wide.hip"""
    nnz, graded = case
    g = _gen(K, Nout, N, kind, nnz, graded, 1)
    ldx, ldc = K + 4, Nout + 4
    Xr, Wc = _operands(N, Nout, K, nnz, g)
    r, c, scale = _scales(N, Nout, graded, g)
    Xr, Wc = X.scale_by(Xr, r, 0), X.scale_by(Wc, c, 1)
    want = X.kept6(Xr, Wc, scale)
    if kind == 0:
        ldw = K + 256                                                  # the product uses the first K columns of W [Nout, ldw]
        W = X.lattice3((Nout, ldw), g)
        W[:, :K] = Wc.t()
        pitch = ldw // 16
    else:
        W, pitch = Wc.contiguous(), 0
    Wf = ops.split_planes_frag(W, kind)
    C = torch.full((N, ldc), 7.0, device=DEV)
    call("pm_rows_times_weight_longk", ptr(_padded(Xr, ldx)), ldx, N, K, ptr(Wf), kind, pitch, Nout, ptr(C), ldc, stream())
    assert torch.equal(C[:, :Nout].double(), want)
    assert bool((C[:, Nout:] == 7.0).all())


# (700 rows on one 128 x 128 tile: ceil(700 / 256) = 3 K slices added by atomics; 700 <= 6 * 128, so nnz = 6 covers every k)
@each_case
@pytest.mark.parametrize("K,M,Nn,lda,ldb,ldc", [(300, 128, 128, 132, 136, 128), (5, 128, 256, 128, 256, 260), (700, 128, 128, 128, 128, 132)])
def test_rows_tn_weight_grad(K, M, Nn, lda, ldb, ldc, case):
    """`pm_rows_tn_weight_grad`: C += A^T B and colsum_a += column sums of A, both accumulating; columns of C beyond Nn
    untouched; the columns of A are the sparse slices, so its column sums are exact too"""
    nnz, graded = case
    g = _gen(K, M, Nn, nnz, graded)
    Ar, Bc = _operands(M, Nn, K, nnz, g, side="row")
    r, c, scale = _scales(M, Nn, graded, g)
    Ar, Bc = X.scale_by(Ar, r, 0), X.scale_by(Bc, c, 1)
    A, B = _padded(Ar.t().contiguous(), lda), _padded(Bc, ldb)
    base = X.base_lattice((M, Nn), g)
    base = base if scale is None else (base.double() * scale).float()
    cs0 = X.scale_by(X.base_lattice((M,), g), r, 0)
    want = _fp32(base.double() + X.kept6(Ar, Bc, scale))
    for with_sums in (True, False):
        C = torch.full((M, ldc), 7.0, device=DEV)
        C[:, :Nn] = base
        cs = cs0.clone()
        call("pm_rows_tn_weight_grad", ptr(A), lda, M, ptr(B), ldb, Nn, K, ptr(C), ldc, ptr(cs) if with_sums else None, stream())
        assert torch.equal(C[:, :Nn].double(), want)
        assert bool((C[:, Nn:] == 7.0).all())
        if with_sums:
            assert torch.equal(cs.double(), _fp32(cs0.double() + Ar.double().sum(1)))


# ------------------------------------------------------------------ the three GCL products from planes
_BATCHES = {}


def _batch(key):
    """(batch on the device, plan, N, trel [N], keep [N, 4] bool: the blocks of A' / dA' that are defined for a row)"""
    if key not in _BATCHES:
        cpu = {"3": lambda: synthetic_batch(3, 2, p=0.3, seed=19), "1": lambda: synthetic_batch(1, 2, p=0.12, seed=19),
               "split": lambda: synthetic_batch(256, 2, p=0.25, seed=1235)}[key]()      # "split": 258 row tiles, two run as halves
        b = cpu.to(DEV)
        plan = ops.plan_build(b.edge_index, b.edge_type, b.edge_dist, b.bars, b.batch, b.is_drum, b.tokens, b.n_bars,
                              b.s_tensor.shape[0])
        N = cpu.num_nodes
        dst, et = cpu.edge_index[1], cpu.edge_type
        keep = torch.ones(N, 4, dtype=torch.bool)
        keep[:, 1], keep[:, 2] = False, False
        keep[dst[et == 4], 1] = True
        keep[dst[et == 5], 2] = True
        _BATCHES[key] = (b, plan, N, plan.field("node_trel").long()[:N], keep.to(DEV))
    return _BATCHES[key]


def _blocks(keep, d):
    return keep[:, :, None].expand(-1, -1, d).reshape(keep.shape[0], 4 * d)


def _wn(W, t, d):
    return torch.cat([W[t * d:(t + 1) * d], W[4 * d:]])


GCL_CASES = [(d, b) for d in (128, 256, 512) for b in ("3", "1")]


@each_case
@pytest.mark.parametrize("B", ["3", "1", "split"])
def test_gcl_forward_from_planes(B, case):
    """h = A' [W_t; W_4; W_5; root] + bias, the aggregate read from planes (d = 512: the only width this entry has); the
    aggregate's zero blocks are zero; with and without row classes; column sums of h as fp64"""
    nnz, graded = case
    d = 512
    b, plan, N, trel, keep = _batch(B)
    g = _gen(d, N, nnz, graded)
    A = X.sparsify(X.lattice3((N, 4 * d), g), 1, nnz, cover=nnz * N >= 4 * d)
    A = torch.where(_blocks(keep, d), A, torch.zeros_like(A))
    W = X.lattice3((7 * d, d), g)
    r, c, scale = _scales(N, d, graded, g, bias=True)
    A, W = X.scale_by(A, r, 0), X.scale_by(W, c, 1)
    bias = X.scale_by(X.base_lattice((d,), g), c, 0)
    want = torch.empty(N, d, dtype=torch.float64, device=DEV)
    for t in range(4):
        m = trel == t
        if bool(m.any()):
            want[m] = X.kept6(A[m], _wn(W, t, d), None if scale is None else scale[m]) + bias.double()
    want = _fp32(want)
    Ap, Wf = ops.split_planes(A), ops.split_planes_frag(W, 1)
    for use_classes in (True, False):
        s = torch.zeros(8, 2, d, dtype=torch.float64, device=DEV)
        h = ops.gcl_forward_from_planes(Ap, plan, d, Wf, bias, col_stats=s, use_classes=use_classes)
        assert torch.equal(h.double(), want)
        assert rel_err(s.sum(0)[0], h.double().sum(0)) < 1e-12 and rel_err(s.sum(0)[1], (h.double() ** 2).sum(0)) < 1e-12


@each_case
@pytest.mark.parametrize("d,B", GCL_CASES + [(256, "split")])
def test_gcl_input_grad_fused(d, B, case):
    """dA' = dh [W_t; W_4; W_5; root]^T on the blocks the segment-reduce backward reads; rows of dh sparse"""
    nnz, graded = case
    b, plan, N, trel, keep = _batch(B)
    g = _gen(d, N, nnz, graded, 1)
    dh = X.sparsify(X.lattice3((N, d), g), 1, nnz, cover=nnz * N >= d)
    W = X.lattice3((7 * d, d), g)
    r, c, _ = _scales(N, 4 * d, graded, g)
    dh, W = X.scale_by(dh, r, 0), X.scale_by(W, torch.cat([c[:d]] * 4 + [c[d:]]), 0)
    want = torch.empty(N, 4 * d, dtype=torch.float64, device=DEV)
    for t in range(4):
        m = trel == t
        if bool(m.any()):
            want[m] = X.kept6(dh[m], _wn(W, t, d).t().contiguous(), (r[m, None] * c[None, :]) if graded else None)
    dhp, Wft = ops.split_planes(dh), ops.split_planes_frag(W, 0)
    kb = _blocks(keep, d)
    for use_classes in (True, False):
        dA = ops.gcl_input_grad_fused(dhp, plan, d, Wft, use_classes=use_classes, out=torch.full((N, 4 * d), NAN, device=DEV))
        assert torch.equal(dA[kb].double(), want[kb])


@each_case
@pytest.mark.parametrize("d,B", GCL_CASES)
def test_gcl_weight_grad_fused(d, B, case):
    """dW += A'^T dh per track relation / over all rows; the columns of A' are the sparse slices (K = the node dimension, K
    slices by atomics); the aggregate's zero blocks are zero"""
    nnz, graded = case
    b, plan, N, trel, keep = _batch(B)
    g = _gen(d, N, nnz, graded, 2)
    A = X.sparsify(X.lattice3((N, 4 * d), g), 0, nnz, cover=True)
    A = torch.where(_blocks(keep, d), A, torch.zeros_like(A))
    dh = X.lattice3((N, d), g)
    r, c, _ = _scales(4 * d, d, graded, g)
    A, dh = X.scale_by(A, r, 1), X.scale_by(dh, c, 1)
    r7 = torch.cat([r[:d]] * 4 + [r[d:]])
    base = (X.base_lattice((7 * d, d), g).double() * r7[:, None] * c[None, :]).float()
    want = _fp32(base.double() + _gcl_dw_model(A, dh, trel, d, r, c, graded))
    Ap, dhp = ops.split_planes(A), ops.split_planes(dh)
    for use_classes in (True, False):
        dW = ops.gcl_weight_grad_fused(Ap, dhp, plan, d, base.clone(), use_classes=use_classes)
        assert torch.equal(dW.double(), want)


# ------------------------------------------------------------------ pm_unembed_dh
@each_case
@pytest.mark.parametrize("d,B,S,drums", [(128, 3, 15, "mixed"), (256, 6, 5, "none"), (256, 6, 5, "all"), (512, 3, 4, "mixed")])
def test_unembed_input_gradient(d, B, S, drums, case):
    """dH = d_logits @ W of the three un-embeddings in one launch; each (node, slot) row of d_logits carries nnz non-zeros
    among its 131 pitch logits and nnz among its 99 duration logits (two separate contractions)"""
    nnz, graded = case
    cpu = synthetic_batch(B, 2, p=0.3, seed=29)
    if drums != "mixed":
        cpu.is_drum = torch.full_like(cpu.is_drum, drums == "all")
    b = cpu.to(DEV)
    plan = ops.plan_build(b.edge_index, b.edge_type, b.edge_dist, b.bars, b.batch, b.is_drum, b.tokens, b.n_bars,
                          b.s_tensor.shape[0], n_slots=S)
    N, dh = cpu.num_nodes, d // 2
    g = _gen(d, B, S, nnz, graded, drums == "all")
    R = N * S
    r, c, _ = _scales(R, d, graded, g)
    sc = (lambda lo, hi: r[:, None] * c[None, lo:hi]) if graded else (lambda lo, hi: None)
    dlp = X.scale_by(X.sparsify(X.lattice3((R, 131), g), 1, nnz), r, 0)
    dld = X.scale_by(X.sparsify(X.lattice3((R, 99), g), 1, nnz), r, 0)
    Wd, Wn = (X.scale_by(X.lattice3((131, dh), g), c[:dh], 1) for _ in range(2))
    Wu = X.scale_by(X.lattice3((99, dh), g), c[dh:], 1)
    dl = torch.cat([dlp, dld], 1).view(N, S, 230).contiguous()
    scratch = torch.empty(int(lib().pm_unembed_dh_scratch_bytes(d)), dtype=torch.uint8, device=DEV)
    dH = torch.full((N, S, d), NAN, device=DEV)
    for prep in (1, 0):
        call("pm_unembed_dh", ptr(dl), ptr(Wd), ptr(Wn), ptr(Wu), ptr(plan.buf), N, plan.E, plan.G, d, S, ptr(dH), ptr(scratch),
             prep, stream())
    drum = b.is_drum.bool()[:, None].expand(N, S).reshape(R)
    want = torch.empty(R, d, dtype=torch.float64, device=DEV)
    want[:, :dh] = torch.where(drum[:, None], X.kept6(dlp, Wd, sc(0, dh)), X.kept6(dlp, Wn, sc(0, dh)))
    want[:, dh:] = X.kept6(dld, Wu, sc(dh, d))
    assert torch.equal(dH.view(R, d).double(), want)


# ------------------------------------------------------------------ the fp16 pair format
PAIR_S = 4096.0              # the scale the lattice implies: value = u / 2^12, so u = value * PAIR_S splits into hi + lo exactly


def _pair_weight_frag(Wu, kind):
    """fragment-major pair planes of the weight whose scaled values are `Wu` (pm_split_planes_frag_h2 at scale 2^12)"""
    rows, cols = Wu.shape
    W = (Wu.double() / PAIR_S).float()
    assert torch.equal(W.double() * PAIR_S, Wu.double())
    out = torch.zeros(1, rows * cols * 3, dtype=torch.int16, device=DEV)
    call("pm_split_planes_frag_h2", ptr(W), rows, cols, kind, 1, rows * cols, rows * cols * 3, PAIR_S, ptr(out), stream())
    return out


@pytest.mark.parametrize("nnz", X.NNZ)
@pytest.mark.parametrize("B", ["3", "1"])
def test_pair_gcl_input_grad_fused(B, nnz):
    """`pm_gcl_input_grad_fused_h2` (d = 512, the only width it has): dh planes encoded here (hi, lo, zero), the weight through
    `pm_split_planes_frag_h2`; dA' = (hi hi + hi lo + lo hi) / (dh scale x weight scale)"""
    d = 512
    b, plan, N, trel, keep = _batch(B)
    g = _gen(d, N, nnz, 3)
    clamps0 = _lib_mod.h2_clamp_events()
    dh = X.sparsify(X.pair_lattice((N, d), g), 1, nnz, cover=nnz * N >= d)
    W = X.pair_lattice((7 * d, d), g)
    want = torch.empty(N, 4 * d, dtype=torch.float64, device=DEV)
    for t in range(4):
        m = trel == t
        if bool(m.any()):
            want[m] = X.kept3(dh[m], _wn(W, t, d).t().contiguous()) / (PAIR_S * PAIR_S)
    D2 = X.pair_planes(dh).contiguous()
    Wft2 = _pair_weight_frag(W, 0)
    sdh = torch.full((1,), PAIR_S, device=DEV)
    kb = _blocks(keep, d)
    for use_classes in (1, 0):
        dA = torch.full((N, 4 * d), NAN, device=DEV)
        call("pm_gcl_input_grad_fused_h2", ptr(D2), N * d, ptr(plan.buf), N, plan.E, plan.G, d, ptr(Wft2), use_classes, ptr(dA),
             ptr(sdh), PAIR_S, stream())
        assert torch.equal(dA[kb].double(), want[kb])
    assert _lib_mod.h2_clamp_events() == clamps0


@pytest.mark.parametrize("nnz", X.NNZ)
@pytest.mark.parametrize("B", ["3", "1"])
def test_pair_gcl_weight_grad_fused(B, nnz):
    """`pm_gcl_weight_grad_fused_h2` at d = 256 from two pair-format plane sets encoded here; accumulates into dW"""
    d = 256
    b, plan, N, trel, keep = _batch(B)
    g = _gen(d, N, nnz, 4)
    clamps0 = _lib_mod.h2_clamp_events()
    A = X.sparsify(X.pair_lattice((N, 4 * d), g), 0, nnz, cover=True)
    A = torch.where(_blocks(keep, d), A, torch.zeros_like(A))
    dh = X.pair_lattice((N, d), g)
    base = X.base_lattice((7 * d, d), g)
    want = _fp32(base.double() + _gcl_dw_model(A, dh, trel, d, None, None, False, kept=lambda a, b_, s: X.kept3(a, b_)) / (PAIR_S * PAIR_S))
    P2, D2 = X.pair_planes(A).contiguous(), X.pair_planes(dh).contiguous()
    sA, sdh = torch.full((1,), PAIR_S, device=DEV), torch.full((1,), PAIR_S, device=DEV)
    for use_classes in (1, 0):
        dW = base.clone()
        call("pm_gcl_weight_grad_fused_h2", ptr(P2), N * 4 * d, ptr(D2), N * d, ptr(plan.buf), N, plan.E, plan.G, d, use_classes,
             ptr(dW), ptr(sA), ptr(sdh), stream())
        assert torch.equal(dW.double(), want)
    assert _lib_mod.h2_clamp_events() == clamps0
