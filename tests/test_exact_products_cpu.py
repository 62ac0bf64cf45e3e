"""The lattice of tests/exact_util.py, checked without a GPU: the generators split into the designed terms, the kept-product
models equal an fp32 accumulation in any term order (so a kernel's accumulation order cannot matter), leaving out any one
product or misreading one plane changes the output words, and two-term lattice products are the fp64 product."""
import pytest
import torch

import exact_util as X

SHAPES = [(130, 132, 36), (260, 68, 1028)]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) + 17)


def _operands(M, N, K, nnz, graded, lattice=X.lattice3):
    g = _gen(M, N, K, nnz, int(graded))
    A = X.sparsify(lattice((M, K), g), 1, nnz, cover=nnz * M >= K)
    B = lattice((K, N), g)
    scale = None
    if graded:
        plain = X.kept6(A, B) if lattice is X.lattice3 else X.exact_mm(A, B)
        A, r = X.grade(A, 0, g)
        B, c = X.grade(B, 1, g)
        scale = r[:, None] * c[None, :]
        model = X.kept6(A, B, scale) if lattice is X.lattice3 else X.exact_mm(A, B, scale)
        assert torch.equal(model, plain * scale)                     # the model scales bit for bit
    return A, B, scale


def test_generators_split_into_the_designed_terms():
    g = _gen(1)
    x = X.lattice3((64, 257), g)
    x1, x2, x3 = X.split3_cpu(x)
    assert set(x1.abs().unique().tolist()) == {1.0, 1.5}
    assert set(x2.abs().unique().tolist()) == {0.0, 2.0 ** -9}
    assert set(x3.abs().unique().tolist()) == {0.0, 2.0 ** -17}
    assert bool((x3[x2 == 0] == 0).all())                            # b <= a
    assert bool((torch.sign(x2)[x2 != 0] == torch.sign(x1)[x2 != 0]).all()) and bool((torch.sign(x3)[x3 != 0] == torch.sign(x1)[x3 != 0]).all())
    assert torch.equal(x1 + x2 + x3, x.double())
    y = X.lattice2((64, 257), g)
    y1, y2, y3 = X.split3_cpu(y)
    assert bool((y3 == 0).all()) and set(y2.abs().unique().tolist()) == {0.0, 2.0 ** -9}
    u = X.pair_lattice((64, 257), g)
    hi, lo = X.split2h_cpu(u)
    assert set(hi.abs().unique().tolist()) == {4096.0, 6144.0} and set(lo.abs().unique().tolist()) == {0.0, 1.0}
    assert bool((torch.sign(lo)[lo != 0] == torch.sign(hi)[lo != 0]).all())
    q = X.base_lattice((1000,), g)
    assert float(q.abs().max()) == 2.0 and torch.equal(q * 4, (q * 4).round())
    # truncation splits the lattice the same way (a kernel may split either way)
    trunc = lambda t: (t.float().view(torch.int32) & -65536).view(torch.float32)
    t1 = trunc(x)
    t2 = trunc(x - t1)
    assert torch.equal(t1.double(), x1) and torch.equal(t2.double(), x2) and torch.equal((x - t1 - t2).double(), x3)
    # the plane encoders restate the splits bit for bit
    p = X.bf16_planes(x)
    assert torch.equal(sum(p[k].view(torch.bfloat16).double() for k in range(3)).view_as(x), x.double())
    p = X.pair_planes(u)
    assert torch.equal((p[0].view(torch.float16).double() + p[1].view(torch.float16).double()).view_as(u), u.double())
    assert int(p[2].abs().max()) == 0


def test_sparsify_and_grade():
    g = _gen(2)
    x = X.lattice3((40, 36), g)
    for nnz in X.NNZ:
        s = X.sparsify(x, 1, nnz)
        assert bool(((s != 0).sum(1) == nnz).all()) and bool((s != 0).any(0).all())
        assert torch.equal(s[s != 0], x[s != 0])
        t = X.sparsify(x.t().contiguous(), 0, nnz)
        assert torch.equal(t, s.t())
        nz = [set(torch.nonzero(s[i]).flatten().tolist()) for i in range(3)]
        assert {(k + 1) % 36 for k in nz[0]} == nz[1]                 # consecutive slices shift by one k
    with pytest.raises(AssertionError):
        X.sparsify(X.lattice3((10, 36), g), 1, 1)                    # 10 slices cannot cover 36 k at nnz = 1
    y, sc = X.grade(x, 0, g)
    assert float(sc.min()) == 2.0 ** -20 and float(sc.max()) == 2.0 ** 20
    assert torch.equal(y.double(), x.double() * sc[:, None])
    assert bool((y.abs() >= 2.0 ** -126).all())
    y1, y2, y3 = X.split3_cpu(y)                                     # the scale goes through the split term by term
    x1, x2, x3 = X.split3_cpu(x)
    assert torch.equal(y3, x3 * sc[:, None]) and torch.equal(y2, x2 * sc[:, None])


def _fp32_accumulate(termsA, termsB, order):
    """sum over `order` (indices into the list of (plane pair, k)) of a[:, k] b[k, :], one fp32 add at a time"""
    K = termsA[0][0].shape[1]
    acc = torch.zeros(termsA[0][0].shape[0], termsB[0][0].shape[1], dtype=torch.float32)
    for t in order.tolist():
        p, k = divmod(t, K)
        a, b = termsA[p][0], termsB[p][0]
        acc = acc + a[:, k, None] * b[None, k, :]                    # an exact fp32 product, one rounding in the add
    return acc


@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("nnz", X.NNZ)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_kept6_equals_fp32_accumulation_in_any_order(M, N, K, nnz, graded):
    A, B, scale = _operands(M, N, K, nnz, graded)
    model = X.kept6(A, B, scale)
    a, b = [t.float() for t in X.split3_cpu(A)], [t.float() for t in X.split3_cpu(B)]
    tA, tB = [(a[i],) for i, _ in X.KEPT6], [(b[j],) for _, j in X.KEPT6]
    g = _gen(M, K, nnz, 5)
    for _ in range(3):
        order = torch.randperm(6 * K, generator=g)
        assert torch.equal(_fp32_accumulate(tA, tB, order).double(), model)


@pytest.mark.parametrize("nnz", X.NNZ)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_pair_kept3_equals_fp32_accumulation_in_any_order(M, N, K, nnz):
    A, B, _ = _operands(M, N, K, nnz, False, X.pair_lattice)
    model = X.kept3(A, B)
    (ha, la), (hb, lb) = X.split2h_cpu(A), X.split2h_cpu(B)
    tA, tB = [(ha.float(),), (ha.float(),), (la.float(),)], [(hb.float(),), (lb.float(),), (hb.float(),)]
    g = _gen(M, K, nnz, 6)
    for _ in range(3):
        assert torch.equal(_fp32_accumulate(tA, tB, torch.randperm(3 * K, generator=g)).double(), model)


@pytest.mark.parametrize("nnz,least", [(1, 0.20), (6, 0.60)])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_leaving_out_one_product_changes_the_outputs(M, N, K, nnz, least):
    """emulated: each third-order product 24-27 % of the words at nnz = 1, ~50 % each second-order one, 100 % x1 y1;
    65-96 % at nnz = 6; the bounds are those less a margin for the draw"""
    A, B, _ = _operands(M, N, K, nnz, False)
    model = X.kept6(A, B)
    for term in X.KEPT6:
        changed = float((X.kept6(A, B, drop=(term,)) != model).double().mean())
        assert changed >= least, (term, changed)
    A, B, _ = _operands(M, N, K, nnz, False, X.pair_lattice)
    model = X.kept3(A, B)
    for term in X.KEPT3:
        changed = float((X.kept3(A, B, drop=(term,)) != model).double().mean())
        assert changed >= least, (term, changed)


@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("nnz", X.NNZ)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_two_term_lattice_products_are_the_fp64_product(M, N, K, nnz, graded):
    A, B, scale = _operands(M, N, K, nnz, graded, X.lattice2)
    model = X.exact_mm(A, B, scale)
    assert torch.equal(X.kept6(A, B, scale), model)
    assert torch.equal((A @ B).double(), model)                      # any fp32 evaluation: nothing rounds
    A3, B3, _ = _operands(M, N, K, nnz, False)                       # (the three-term lattice's own product is NOT an fp32 value)
    full = A3.double() @ B3.double()
    assert not torch.equal(full.float().double(), full)


@pytest.mark.parametrize("nnz", X.NNZ)
def test_one_k_column_with_plane_3_read_as_plane_2(nnz):
    """B's third plane replaced by its second in a single k: every output row that is non-zero there (and only those) moves"""
    M, N, K = 130, 132, 36
    A, B, _ = _operands(M, N, K, nnz, False)
    a, b = X.split3_cpu(A), list(X.split3_cpu(B))
    k = 35                                                           # the K tail of every tile size in use
    model = X.kept6(A, B)
    b3 = b[2].clone()
    b3[k] = b[1][k]
    wrong = sum(a[i] @ (b3 if j == 2 else b[j]) for i, j in X.KEPT6)
    rows = A[:, k] != 0
    assert 0 < int(rows.sum()) < M
    moved = (wrong != model).any(1)
    assert torch.equal(moved, rows)
