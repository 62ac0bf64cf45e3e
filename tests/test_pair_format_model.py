"""The CPU emulation of the fp16 pair operand format (tests/pair_format_util.py) against what csrc/common.h documents, with no
GPU: the representation bound element by element over 40 binades, and the three GCL products on the operand constructions
of tests/test_pair_format_gpu.py — the reference of that file's conditions checked alone, on the build host."""
import pytest
import torch

import pair_format_util as pf
from polyphemus_amd.synthetic import synthetic_batch


def test_pow2_scale_restates_the_kernels_formula():
    for bound, want in ((1.0, 2.0 ** 12), (1.5, 2.0 ** 12), (1.9999999, 2.0 ** 12), (2.0, 2.0 ** 11), (2.0 ** 12, 1.0),
                        (2.0 ** 13 - 1, 1.0), (2.0 ** 13, 0.5), (3.0e-5, 2.0 ** 28), (0.0, 1.0), (-1.0, 1.0), (float("inf"), 1.0),
                        (float("nan"), 1.0), (3.1e38, 1.0), (2.0 ** -140, 2.0 ** 120), (2.0 ** -120, 2.0 ** 120), (2.0 ** 120, 2.0 ** -108)):
        assert pf.pow2_scale(bound, 13) == want, (bound, pf.pow2_scale(bound, 13), want)
    for b in (1e-30, 3e-7, 0.7, 1.0, 12345.0, 1e30):           # bound * s in [2^(target-1), 2^target)
        for target in (9, 13):
            assert 2.0 ** (target - 1) <= b * pf.pow2_scale(b, target) < 2.0 ** target


@pytest.mark.parametrize("vmax", [1.0, 1e-6, 1e3, 2.0 ** -60, 2.0 ** 60, 37.0])
def test_representation_bound_element_by_element(vmax):
    """|decode - v| <= max(2^-22 |v s|, 2^-25) / s for every element: magnitudes log-uniform over 2^-40 .. 2^0 of the tensor's
    |max|, random signs, exact zeros and fp32 subnormals among them — the bound csrc/common.h states."""
    g = torch.Generator().manual_seed(7)
    n = 1 << 16
    mag = torch.exp2(-40.0 * torch.rand(n, generator=g, dtype=torch.float64)) * vmax
    v = (mag * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).float()
    v[0] = vmax
    v[1:9] = 0.0
    v[9:17] = torch.tensor([1.0e-45, -1.0e-45, 1.0e-40, -3.0e-39, 5.0e-42, 1.1e-38, -1.1e-38, 7.0e-44])   # fp32 subnormals
    s = pf.pow2_scale(float(v.abs().max()), 13)
    assert 2.0 ** 12 <= float(v.abs().max()) * s < 2.0 ** 13
    err = (pf.decode(v, s) - v.double()).abs()
    bound = pf.rep_bound(v.double().abs() * s) / s
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((pf.decode(v, s)[1:9]).abs().max()) == 0.0
    # ... and neither half of the bound is slack by more than a factor of four: both are reached
    vs = v.double().abs() * s
    assert float((err / bound)[vs >= 0.25].max()) > 0.25 and float((err / bound)[(vs < 0.25) & (vs > 2.0 ** -20)].max()) > 0.25


@pytest.fixture(scope="module")
def graph():
    cpu = synthetic_batch(16, 2, p=0.3, seed=29)
    return cpu, pf.trel_of(cpu)


@pytest.mark.parametrize("t", [0, 4, 8])
@pytest.mark.parametrize("d,p", [(128, 0.0), (256, 0.1), (512, 0.1)])
def test_emulated_products_alone_hold_the_conditions(graph, d, p, t):
    """The emulation (exact accumulation, lo * lo dropped) of forward, input gradient and weight gradient on the operands of
    the GPU test, against the fp64 contraction of the same fp32 operands: within max(2 * fp32 product's error, 2^-22) up to
    2^8 of dynamic range — an fp32 matmul stands where the kernels' exact-split route stands on the GPU."""
    cpu, trel = graph
    o = pf.Operands(cpu.num_nodes, d, t=t)
    A32 = pf.aggregate64(o.x.double(), o.T.double(), cpu, trel, p, 5, 2).float()
    dh32 = pf.bn_bwd64(o.hpre, o.du, o.mean, o.var, o.gamma, o.beta).float()
    sa, sdh = o.agg_scale(p), o.dh_scale()
    assert float(A32.abs().max()) * sa < 2.0 ** 13 and float(dh32.abs().max()) * sdh < 2.0 ** 13
    keep = pf.keep_blocks(cpu, d)
    masks = pf.compared(o, keep)
    ref = pf.plain_products(o, A32, dh32, trel)
    e32 = pf.errors(pf.plain_products(o, A32, dh32, trel, pf.mm32), ref, masks)
    em = pf.errors(pf.model_products(o, A32, dh32, trel, sa, sdh), ref, masks)
    for k in ref:
        print(f"d={d} t=2^{t} {k}: model {em[k]:.2e} fp32 {e32[k]:.2e}")
        assert em[k] <= pf.condition(t, False, 0.0, e32[k], 0.0), (k, em[k], e32[k])


def test_the_model_condition_bites():
    """Beyond 2^8 the GPU test holds the kernels to what the emulation explains; that is a check only if the emulation moves
    when the format does: dropping one cross product, or flushing fp16 subnormals, changes its error by far more than the
    condition's factor of two."""
    cpu = synthetic_batch(16, 2, p=0.3, seed=29)
    trel, d, t = pf.trel_of(cpu), 128, 12
    o = pf.Operands(cpu.num_nodes, d, t=t)
    A32 = pf.aggregate64(o.x.double(), o.T.double(), cpu, trel, 0.0, 5, 2).float()
    dh32 = pf.bn_bwd64(o.hpre, o.du, o.mean, o.var, o.gamma, o.beta).float()
    sa, sdh = o.agg_scale(0.0), o.dh_scale()
    masks = pf.compared(o, pf.keep_blocks(cpu, d))
    ref = pf.plain_products(o, A32, dh32, trel)
    em = pf.errors(pf.model_products(o, A32, dh32, trel, sa, sdh), ref, masks)
    no_lh = pf.errors(pf.model_products(o, A32, dh32, trel, sa, sdh, terms=("hh", "hl")), ref, masks)
    ftz = pf.errors(pf.model_products(o, A32, dh32, trel, sa, sdh, flush=True), ref, masks)
    for k in ref:
        print(f"{k}: model {em[k]:.2e} without lo*hi {no_lh[k]:.2e} flushed {ftz[k]:.2e}")
        assert no_lh[k] > 10 * em[k] and ftz[k] > 10 * em[k], k
