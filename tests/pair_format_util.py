"""CPU emulation of the fp16 pair operand format (PmH2, include/polyphemus_hip.h; pm_pow2_scale / pm_split2h_pair of
csrc/common.h), its representation bound, the three GCL products as fp64 contractions, and the operand constructions that
tests/test_pair_format_model.py (CPU) and tests/test_pair_format_gpu.py (the kernels) share.  Pure torch / numpy."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from util import dropout_keep_np

F16_MAX = 65504.0
TARGET = 13                  # max |v s| lands in [2^12, 2^13) when the bound is the tensor's own |max|
DH_FACTOR = 16.0             # dh bound = max_c |gamma_c rstd_c| * |du|max * 16   (gcl.hip k_gcl_dagg, norm.hip k_bn_bwd_apply4_sums)
W_SCALE = 16.0               # kH2WScale of vae_step.hip: the scale the step builds its weight planes with
FLOOR = 2.0 ** -22           # "a second form of the same kernel" (tests/test_dp_forms_gpu.py)


# ---------------------------------------------------------------------------------------------- the format
def pow2_scale(bound, target=TARGET):
    """pm_pow2_scale: the power of two s with bound * s in [2^(target-1), 2^target); 1 for a zero / non-finite bound.
    `bound` is an fp32 value (anything else is rounded to fp32 first, as the kernel's argument is)."""
    b = np.float32(bound)
    if not (b > 0) or not (b < np.float32(3.0e38)):
        return 1.0
    e = int((b.view(np.uint32) >> 23) & 0xFF) - 126            # bound in [2^(e-1), 2^e); fp32 subnormals: e = -126
    k = max(-120, min(120, target - e))
    return 2.0 ** k


def split(v32, s, flush=False):
    """pm_split2h_pair of v * s (fp32 multiply, clamped to fp16's range as the kernels that can saturate do): (hi, lo) as fp64.
    torch's CPU fp16 conversions round to nearest even and keep subnormals; `flush` zeroes fp16 subnormals instead (what a
    conversion or a matrix core in flush-to-zero mode would do — the tests' counter-model)."""
    a = (v32.to(torch.float32) * torch.tensor(s, dtype=torch.float32)).clamp(-F16_MAX, F16_MAX)
    hi = a.to(torch.float16)
    lo = (a - hi.float()).to(torch.float16)                    # the residual is exact in fp32
    if flush:
        tiny = 2.0 ** -14
        hi = torch.where(hi.float().abs() < tiny, torch.zeros_like(hi), hi)
        lo = torch.where(lo.float().abs() < tiny, torch.zeros_like(lo), lo)
    return hi.double(), lo.double()


def decode(v32, s):
    hi, lo = split(v32, s)
    return (hi + lo) / s


def rep_bound(vs_abs):
    """common.h's representation bound in units of the SCALED value: 2^-22 |v s| while lo is a normal fp16, 2^-25 below that."""
    vs_abs = torch.as_tensor(vs_abs, dtype=torch.float64)
    return torch.maximum(vs_abs * 2.0 ** -22, torch.full_like(vs_abs, 2.0 ** -25))


def pair_product(A, B, sa, sb, terms=("hh", "hl", "lh"), flush=False):
    """(hi_a hi_b + hi_a lo_b + lo_a hi_b) / (sa sb) in fp64 for fp32 operands A [m, k], B [k, n] (lo * lo is dropped, as in
    the kernels).  `terms` lets a test drop one of the three products."""
    ha, la = split(A, sa, flush)
    hb, lb = split(B, sb, flush)
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64)
    if "hh" in terms:
        out += ha @ hb
    if "hl" in terms:
        out += ha @ lb
    if "lh" in terms:
        out += la @ hb
    return out / (sa * sb)


def mm64(A, B):
    return A.double() @ B.double()


def mm32(A, B):
    return (A.float() @ B.float()).double()


def pair_mm(sa, sb, **kw):
    return lambda A, B: pair_product(A, B, sa, sb, **kw)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float((a - b).norm())


def octave_errors(pair, triple, ref, s):
    """per magnitude octave of |ref s| (everything below 2^-40 in one): [(upper end, max |pair - ref| s, allowed)] with
    allowed = the representation bound at the octave's upper end + 2 max |triple - ref| s over the same octave — the second
    term is the fp32 evaluation both routes share, taken from the exact-split route"""
    pair, triple, ref = (t.double().flatten().cpu() * s for t in (pair, triple, ref))
    lo_oct, n_oct = -40, 40 + 18
    octv = (torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** lo_oct))).long() - lo_oct).clamp(0, n_oct - 1)
    ep = torch.zeros(n_oct, dtype=torch.float64).scatter_reduce_(0, octv, (pair - ref).abs(), "amax")
    et = torch.zeros(n_oct, dtype=torch.float64).scatter_reduce_(0, octv, (triple - ref).abs(), "amax")
    cnt = torch.bincount(octv, minlength=n_oct)
    return [(2.0 ** (o + lo_oct + 1), float(ep[o]), float(rep_bound(2.0 ** (o + lo_oct + 1))) + 2.0 * float(et[o]))
            for o in range(n_oct) if int(cnt[o]) > 0]


# ---------------------------------------------------------------------------------------------- the layer, fp64
def aggregate64(x, T, batch, trel, p, seed, layer):
    """A' [N, 4d] of the compact layout: [mean message of the node's track relation | onset | next | x], GCL.message +
    scatter-mean of the reference (model.py:110,123-135) in the dtype of `x`, with the kernels' message dropout."""
    N, d = x.shape
    src, dst = batch.edge_index[0], batch.edge_index[1]
    parts = []
    for r in range(6):
        m = batch.edge_type == r
        msg = F.relu(x[src[m]] * T[batch.edge_dist[m].long()])
        if p > 0:
            eids = torch.nonzero(m).flatten().numpy()
            msg = msg * torch.from_numpy(dropout_keep_np(seed, layer, eids, d, p)) / (1.0 - p)
        h = torch.zeros(N, d, dtype=x.dtype).index_add_(0, dst[m], msg)
        cnt = torch.zeros(N, dtype=x.dtype).index_add_(0, dst[m], torch.ones(int(m.sum()), dtype=x.dtype))
        parts.append(h / cnt.clamp(min=1).unsqueeze(1))
    ref = torch.stack(parts, 1)
    return torch.cat([ref[torch.arange(N), trel.long()], ref[:, 4], ref[:, 5], x], 1)


def trel_of(batch):
    """the track relation (0..3) of each node's incoming track edges; 0 for a node without any (a CPU stand-in for the plan's
    node_trel where no plan is built)"""
    trel = torch.zeros(batch.num_nodes, dtype=torch.long)
    m = batch.edge_type < 4
    trel[batch.edge_index[1][m]] = batch.edge_type[m].long()
    return trel


def keep_blocks(batch, d):
    """[N, 4d] mask of the dA' blocks the kernels write: the onset / next block only for rows that have such edges"""
    N = batch.num_nodes
    dst, et = batch.edge_index[1], batch.edge_type
    on, nx = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    on[dst[et == 4]] = True
    nx[dst[et == 5]] = True
    keep = torch.ones(N, 4, d, dtype=torch.bool)
    keep[~on, 1] = False
    keep[~nx, 2] = False
    return keep.view(N, 4 * d)


def bn_bwd64(hpre, du, mean, var, gamma, beta, eps=1e-5, relu=True):
    """dh of BatchNorm (+ ReLU) backward on batch statistics, fp64 (pm_bn_bwd_elem)"""
    h, du, mean, var, gamma, beta = (t.double() for t in (hpre, du, mean, var, gamma, beta))
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (h - mean) * rstd
    if relu:
        du = torch.where(xh * gamma + beta > 0, du, torch.zeros_like(du))
    return gamma * rstd * (du - du.mean(0) - xh * (du * xh).mean(0))


def _wn(W, t, d):
    return torch.cat([W[t * d:(t + 1) * d], W[4 * d:]])


def gcl_forward(mm, A, W, trel, d):
    """h [N, d] = A'[n] @ [W_trel(n); W_4; W_5; root]  (no bias)"""
    h = torch.zeros(A.shape[0], d, dtype=torch.float64)
    for t in range(4):
        r = trel == t
        if bool(r.any()):
            h[r] = mm(A[r], _wn(W, t, d))
    return h


def gcl_input_grad(mm, dh, W, trel, d):
    """dA' [N, 4d] = dh[n] @ [W_trel(n); W_4; W_5; root]^T"""
    dA = torch.zeros(dh.shape[0], 4 * d, dtype=torch.float64)
    for t in range(4):
        r = trel == t
        if bool(r.any()):
            dA[r] = mm(dh[r], _wn(W, t, d).t().contiguous())
    return dA


def gcl_weight_grad(mm, A, dh, trel, d):
    """dW [7d, d] = A'^T dh per track relation, stacked as the weight"""
    dW = torch.zeros(7 * d, d, dtype=torch.float64)
    for t in range(4):
        r = trel == t
        if bool(r.any()):
            dW[t * d:(t + 1) * d] = mm(A[r, :d].t().contiguous(), dh[r])
    dW[4 * d:] = mm(A[:, d:].t().contiguous(), dh)
    return dW


# ---------------------------------------------------------------------------------------------- operands
def clear_of_pow2(bound, margin=2.0 ** -6):
    """is `bound` at least `margin` (relative) away from the powers of two on both sides?"""
    f = bound / 2.0 ** math.floor(math.log2(bound))            # [1, 2)
    return f >= 1.0 + margin and f <= 2.0 * (1.0 - margin)


def dh_bound64(gamma, var, du_absmax, eps=1e-5):
    return float((gamma.double().abs() / torch.sqrt(var.double() + eps)).max()) * float(du_absmax) * DH_FACTOR


def agg_bound32(x_absmax, t_absmax, p):
    """the aggregate's bound in the kernels' own fp32 arithmetic: |x|max * max(1, |T|max * (1 / (1 - p)))"""
    sc = np.float32(1.0) / (np.float32(1.0) - np.float32(p)) if p > 0 else np.float32(1.0)
    return np.float32(x_absmax) * max(np.float32(1.0), np.float32(t_absmax) * sc)


class Operands:
    """Operands of one GCL layer with a REAL outlier 2^t above the bulk (not a lie in the |max| words):
      x[:, cx] *= 2^t with the rows cx + k d of the [7d, d] weight zeroed, so no output of the forward depends on the outlier
        channel, yet it sets |x|max;
      du[:, cg] *= 2^t (cg != cx) with column cg of the weight zeroed, so no input gradient depends on it;
      the weight gradient sees both and is compared without those rows and that column.
    `heavy`: instead, x and du are randn * 2^(3 randn) elementwise and nothing is excluded.
    `xs`, `gs`: overall magnitudes of x and du."""

    def __init__(self, N, d, t=0, heavy=False, xs=1.0, gs=1.0, seed=11):
        g = torch.Generator().manual_seed(seed * 4099 + d)
        rn = lambda *s: torch.randn(*s, generator=g)
        self.N, self.d, self.t, self.heavy = N, d, t, heavy
        self.cx, self.cg = 5, d - 3
        x, du = rn(N, d), rn(N, d)
        if heavy:
            x, du = x * torch.exp2(3.0 * rn(N, d)), du * torch.exp2(3.0 * rn(N, d))
        else:
            x[:, self.cx] *= 2.0 ** t
            du[:, self.cg] *= 2.0 ** t
        self.x, self.du = (x * xs).contiguous(), (du * gs).contiguous()
        self.T = (rn(d, 32) * 0.5).t().contiguous() + rn(d) * 0.1          # the edge table [32, d]: nn weight^T + bias
        W = rn(7 * d, d) / d ** 0.5
        self.out_rows = torch.ones(7 * d, dtype=torch.bool)                # rows / columns of W that take part in comparisons
        self.out_cols = torch.ones(d, dtype=torch.bool)
        if not heavy:
            W[self.cx::d] = 0.0
            W[:, self.cg] = 0.0
            self.out_rows[self.cx::d] = False
            self.out_cols[self.cg] = False
        self.W = W.contiguous()
        self.bias = rn(d) * xs
        self.hpre = rn(N, d) * 1.5 + 0.3
        self.gamma, self.beta = torch.rand(d, generator=g) + 0.5, rn(d) * 0.2
        self.mean, self.var = self.hpre.mean(0), self.hpre.var(0, unbiased=False)
        # the dh bound at least 2^-6 relative away from a power of two: rsqrtf's rounding cannot move the binade then
        for _ in range(8):
            if clear_of_pow2(self.dh_bound()):
                break
            self.gamma = self.gamma * 1.25
        assert clear_of_pow2(self.dh_bound()), self.dh_bound()

    def dh_bound(self):
        return dh_bound64(self.gamma, self.var, float(self.du.abs().max()))

    def dh_scale(self):
        return pow2_scale(self.dh_bound())

    def agg_scale(self, p):
        return pow2_scale(agg_bound32(float(self.x.abs().max()), float(self.T.abs().max()), p))

    def dW_mask(self):
        return self.out_rows[:, None] & self.out_cols[None, :]


def plain_products(ops_, A32, dh32, trel, mm=mm64):
    """forward (no bias), input gradient and weight gradient of the layer on fp32 operands A' [N, 4d], dh [N, d], ops_.W"""
    d, W = ops_.d, ops_.W
    return {"forward": gcl_forward(mm, A32, W, trel, d), "input_grad": gcl_input_grad(mm, dh32, W, trel, d),
            "weight_grad": gcl_weight_grad(mm, A32, dh32, trel, d)}


def model_products(ops_, A32, dh32, trel, sa, sdh, ws=W_SCALE, **kw):
    """... by the pair emulation run with the scales `sa` (A'), `sdh` (dh) and `ws` (weights)"""
    d, W = ops_.d, ops_.W
    return {"forward": gcl_forward(pair_mm(sa, ws, **kw), A32, W, trel, d),
            "input_grad": gcl_input_grad(pair_mm(sdh, ws, **kw), dh32, W, trel, d),
            "weight_grad": gcl_weight_grad(pair_mm(sa, sdh, **kw), A32, dh32, trel, d)}


def compared(ops_, keep):
    """the outputs each product is compared on: all of h; dA' on the blocks the kernels write; dW without the outlier rows / column"""
    return {"forward": None, "input_grad": keep, "weight_grad": ops_.dW_mask()}


def errors(got, ref, masks):
    return {k: rel_l2(got[k] if masks[k] is None else got[k][masks[k]], ref[k] if masks[k] is None else ref[k][masks[k]]) for k in ref}


def condition(t, heavy, err_pair, err_alt, err_model):
    """the bound of a product's pair-format error: up to 2^8 of dynamic range that of a second form of the same kernel (twice the
    exact-split route's error, floor 2^-22); beyond, and for heavy tails, twice what the documented representation explains"""
    if heavy or t >= 12:
        return 2.0 * (err_model + err_alt)
    return max(2.0 * err_alt, FLOOR)
