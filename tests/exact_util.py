"""Operands on which the split-product kernels have no rounding left, and fp64 statements of what they must return.

An fp32 value enters the matrix-core kernels as three bf16 terms x = x1 + x2 + x3, and six of the nine partial products are
kept (x_i y_j with i + j <= 4).  The fp16 pair format keeps three of four (hi hi, hi lo, lo hi).  On the lattices below every
kept partial product, and every partial sum of them in ANY order, is exactly representable in fp32: accumulation order, K
slices added by atomics, tile schedules and rounding modes drop out, and a kernel must return bit for bit the sum of exactly
the products it claims to keep.  A wrong plane, a skipped product or a misplaced k changes output words.

  three-term lattice  x = s (h + a 2^-9 + b 2^-17),  s in {-1, 1}, h in {1, 1.5}, a in {0, 1}, b in {0, a}:
      round-to-nearest (and truncating) bf16 splitting gives x1 = s h, x2 = s a 2^-9, x3 = s b 2^-17; the six kept products
      are multiples of 2^-18 (the dropped ones, x2 y3, x3 y2, x3 y3, are not needed for that);
  two-term lattice    b = 0: x y itself is a multiple of 2^-18, so the six kept products ARE the product (x2 y2 is kept),
      and an fp32 kernel must equal the fp64 product;
  pair lattice        u = s 2^12 (h + a 2^-12): hi = s 2^12 h, lo = s a; hi hi, hi lo, lo hi are multiples of 2^11.

The operand that indexes the output row carries at most `nnz` non-zeros along the contraction (`sparsify`), the other one is
dense: sum |x||y| <= 6 * 1.50197^2 < 13.6 < 16, so every partial sum is a multiple of 2^-18 below 16: 22 bits (with a lattice
bias / accumulate base q/4, |q| <= 8: below 32, 23 bits).  Exact power-of-two factors per output row and per output column
(`grade`, 2^e with |e| <= 20) scale every term and the result exactly and keep every term a normal number; they close the
max-norm's blindness to rows far below a tensor's maximum.

nnz: 1 needs nothing of the matrix core's adder (every output is one product's kept terms plus zeros).  nnz = 6 needs it to
carry 22 bits below 16.  Largest nnz exact on the MI355X: 6, the largest tried (NNZ_EXACT_ON_HW; every kernel, bf16, fp16 and
fp32 MFMA alike, profiles/LOG.md).

Pure torch; nothing here calls the library under test (tests/pair_format_util.py, reused for the fp16 pair split, is a CPU
emulation too).  Works on CPU and on device tensors alike (the GPU tests build their fp64 models on the device)."""
import torch

from pair_format_util import split as _pair_split

NNZ = (1, 6)
NNZ_EXACT_ON_HW = 6          # largest nnz at which v_mfma_f32_32x32x16_bf16 / _f16 sums were bit-exact on gfx950 (profiles/LOG.md)
BOUND = 16.0                 # sum |x||y| per output stays below this (times the output's scale)
PAIR_BOUND = 2.0 ** 28       # ... in the pair format's scaled units: 6 * 6145^2 < 2^28, unit 2^11: 17 bits


def _bits(shape, gen):
    return torch.randint(0, 2, tuple(shape), generator=gen, dtype=torch.int64, device=gen.device).double()


def lattice3(shape, gen):
    """s (h + a 2^-9 + b 2^-17) as fp32, on the device of the torch.Generator `gen`"""
    s, h, a, b = (_bits(shape, gen) for _ in range(4))
    return ((2.0 * s - 1.0) * (1.0 + 0.5 * h + a * 2.0 ** -9 + a * b * 2.0 ** -17)).float()


def lattice2(shape, gen):
    """s (h + a 2^-9) as fp32"""
    s, h, a = (_bits(shape, gen) for _ in range(3))
    return ((2.0 * s - 1.0) * (1.0 + 0.5 * h + a * 2.0 ** -9)).float()


def pair_lattice(shape, gen):
    """s 2^12 (h + a 2^-12) as fp32: the SCALED value of the fp16 pair format (what hi + lo encode)"""
    s, h, a = (_bits(shape, gen) for _ in range(3))
    return ((2.0 * s - 1.0) * (4096.0 + 2048.0 * h + a)).float()


def base_lattice(shape, gen):
    """bias / accumulate base / residual values: q / 4, integer |q| <= 8"""
    return (torch.randint(-8, 9, tuple(shape), generator=gen, dtype=torch.int64, device=gen.device).double() / 4.0).float()


def sparsify(x, dim, nnz, cover=True):
    """Keeps `nnz` entries per slice along `dim` (the contraction) of a 2-D tensor: slice i keeps the positions
    (i + j ceil(K / nnz)) mod K, j < nnz, so consecutive slices shift by one k.  With at least ceil(K / nnz) slices every k is
    non-zero somewhere: asserted, unless `cover=False` says the caller knows it cannot hold (K > nnz * slices: the nnz = 1
    twin of a long-K case, whose nnz = 6 twin covers every k)."""
    assert x.dim() == 2 and dim in (0, 1)
    K, n = x.shape[dim], x.shape[1 - dim]
    stride = -(-K // nnz)
    i = torch.arange(n, device=x.device).unsqueeze(1)
    pos = (i + torch.arange(min(nnz, K), device=x.device).unsqueeze(0) * stride) % K    # [n, nnz]
    mask = torch.zeros(n, K, dtype=torch.bool, device=x.device)
    mask.scatter_(1, pos, True)
    assert int(mask.sum(1).max()) <= nnz
    if cover:
        assert n >= stride and bool(mask.any(0).all()), f"{n} slices cannot cover K = {K} at nnz = {nnz}"
    mask = mask if dim == 1 else mask.t()
    return torch.where(mask, x, torch.zeros_like(x)).contiguous()


def pow2_scales(n, gen, span=20, lo=None):
    """n exact powers of two 2^e, lo <= e <= span (lo = -span unless given), both ends present when n >= 2 (fp64).
    Rows that meet a bias take lo = 0, span = 16: p r + q/4 is exact in fp32 only while q/4 is a multiple of the product's
    unit 2^-18 r (r <= 2^16) and below 32 r (r >= 1); the column scale multiplies the bias too and is free."""
    lo = -span if lo is None else lo
    e = torch.randint(lo, span + 1, (n,), generator=gen, dtype=torch.int64, device=gen.device)
    if n >= 2:
        e[0], e[n // 2] = lo, span
    return torch.exp2(e.double())


def scale_by(x, sc, dim):
    """x times the fp64 powers of two `sc` along `dim`, as fp32; asserted exact"""
    shape = [1] * x.dim()
    shape[dim] = -1
    want = x.double() * sc.view(shape).to(x.device)
    y = want.float()
    assert torch.equal(y.double(), want)
    return y


def grade(x, dim, gen, span=20, lo=None):
    """(x scaled by an exact power of two per index of `dim`, the fp64 scales [x.shape[dim]])"""
    sc = pow2_scales(x.shape[dim], gen, span, lo)
    return scale_by(x, sc, dim), sc


def split3_cpu(x):
    """torch bf16 round-to-nearest, three terms (fp64 values); the remainder is asserted to be zero"""
    x = x.float()
    x1 = x.bfloat16().float()
    r1 = x - x1
    x2 = r1.bfloat16().float()
    r2 = r1 - x2
    x3 = r2.bfloat16().float()
    assert bool((r2 - x3 == 0).all()), "not a three-term bf16 value"
    return x1.double(), x2.double(), x3.double()


KEPT6 = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))       # (i, j): x_{i+1} y_{j+1}, i + j <= 2


def _check(out, absprod, bound, scale):
    assert torch.equal(out.float().double(), out), "model is not an fp32 value: the operands left the lattice"
    lim = bound if scale is None else bound * scale
    assert bool((absprod < lim).all()), "sum |x||y| reaches the bound: partial sums may round"


def kept6(A, B, scale=None, drop=()):
    """fp64 sum of the six kept products of A [M, K] @ B [K, N] (fp32 operands).  `scale` [M, N] or None: the exact
    power-of-two scale of each output (row scale x column scale of graded operands).  `drop`: terms of KEPT6 to leave out
    (the sensitivity tests).  Asserts that the result is an fp32 value and that sum |A||B| < 16 scale."""
    a, b = split3_cpu(A), split3_cpu(B)
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64, device=A.device)
    for i, j in KEPT6:
        if (i, j) not in drop:
            out += a[i] @ b[j]
    _check(out, A.double().abs() @ B.double().abs(), BOUND, scale)
    return out


def exact_mm(A, B, scale=None):
    """the fp64 product, asserted to be an fp32 value under the same bound (two-term lattice operands)"""
    out = A.double() @ B.double()
    _check(out, A.double().abs() @ B.double().abs(), BOUND, scale)
    return out


def split2h_cpu(u):
    """fp16 pair split of an already scaled value (tests/pair_format_util.split at scale 1): (hi, lo) fp64, remainder zero"""
    hi, lo = _pair_split(u, 1.0)
    assert bool((u.double() - hi - lo == 0).all()), "not a two-term fp16 value"
    return hi, lo


KEPT3 = ("hh", "hl", "lh")


def kept3(A, B, drop=()):
    """fp64 hi hi + hi lo + lo hi of scaled pair operands A [M, K] @ B [K, N] (lo lo is dropped, as in the kernels)"""
    (ha, la), (hb, lb) = split2h_cpu(A), split2h_cpu(B)
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64, device=A.device)
    for name, x, y in (("hh", ha, hb), ("hl", ha, lb), ("lh", la, hb)):
        if name not in drop:
            out += x @ y
    _check(out, A.double().abs() @ B.double().abs(), PAIR_BOUND, None)
    return out


def bf16_planes(x):
    """int16 [3, numel]: the bf16 bit patterns of split3_cpu(x) (what `pm_split_planes` must produce on the lattice)"""
    return torch.stack([t.float().bfloat16().view(torch.int16).reshape(-1) for t in split3_cpu(x)])


def pair_planes(u):
    """int16 [3, numel]: hi and lo as fp16 bit patterns in planes 0 and 1, plane 2 zero (PmH2 operand planes)"""
    hi, lo = split2h_cpu(u)
    p = [t.float().half().view(torch.int16).reshape(-1) for t in (hi, lo)]
    return torch.stack(p + [torch.zeros_like(p[0])])
