"""The bar-resident kernels of the structure CNNs (csrc/cnn.hip: pm_cnn_enc_fwd / pm_cnn_dec_fwd / pm_cnn_enc_bwd, the training
step's default since PM_CNN_FUSED) against two references: fp64 torch on the CPU (conv2d, batch_norm in training mode, max_pool2d,
interpolate, autograd) and the chain of generic launches they replace, through the existing `ops` wrappers.

Bounds.  A convolution of the fused set adds in the order of k_conv3x3_fwd, so c0 and c2 (same input) are `torch.equal` to its
output.  Every other tensor — activations, saved mean / var, running statistics, weight / bias / gamma / beta gradients, dc1, da0,
dc0 — may be at most TWICE as far (relative L2) from the fp64 reference as the generic chain is on the same inputs: both run the
same fp32 arithmetic per element, the margin is for the different association of the fp64 partial sums (and of the fp32 partials
of conv0's weight gradient).  Sizes: G = 1 bar (one partial workgroup), 3 (odd), 67 (several workgroups of one bar: the cross-workgroup sums) and
300 (more bars than the 256 workgroups a launch has at most: 44 of them walk a second bar, as every workgroup does at the bench's 512).  Inputs are 0/1
structure grids, from G = 3 on with an all-zero and an all-one bar: behind the ReLU the pool sees runs of equal zeros, and the
positions of da0 that receive gradient must be torch's (first maximum wins).

The step: PM_CNN_FUSED=1 against =0 at the smallest `hip_fullsize_step` spec of tests/util.py with 8 layers, deterministic mode (what the
test sees is what every run sees), each side against the fp64 oracle: losses, all 152 gradients, the norms' buffers, the same
factor-two rule per tensor; two runs of the fused side are bit-identical."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from util import SMALLSIZE, bn_keys, hip_fullsize_step, oracle_fullsize

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 67, 300)
EPS, MOM = 1e-5, 0.1


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    den = float(b.norm())
    num = float((a - b).norm())
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def check_factor_two(tag, fused, old, ref):
    """every tensor of `fused` at most twice as far from `ref` (fp64) as `old` is; returns the figures"""
    fig = {k: (rel_l2(fused[k], ref[k]), rel_l2(old[k], ref[k])) for k in ref}
    print(tag, json.dumps({k: [float(f"{a:.3e}"), float(f"{b:.3e}")] for k, (a, b) in fig.items()}))
    for k, (a, b) in fig.items():
        assert a <= 2.0 * b, (tag, k, a, b)
    return fig


def structure_grids(G, seed):
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(G, 1, 4, 32, generator=g) < 0.3).float()
    if G >= 3:
        s[0] = 0.0
        s[1] = 1.0
    return s


def encoder_params(seed):
    """conv / norm parameters at the scale of the model's initialisation, gamma / beta moved off 1 / 0; running statistics of a
    model that has taken steps already"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, k=1.0: (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(w0=r(8, 1, 3, 3, k=1 / 3), b0=r(8, k=1 / 3), g1=1 + r(8, k=0.3), be1=r(8, k=0.3),
                w4=r(16, 8, 3, 3, k=72 ** -0.5), b4=r(16, k=72 ** -0.5), g5=1 + r(16, k=0.3), be5=r(16, k=0.3),
                rm1=r(8, k=0.2), rv1=1 + r(8, k=0.3), rm5=r(16, k=0.2), rv5=1 + r(16, k=0.3))


def decoder_params(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape, k=1.0: (torch.rand(*shape, generator=g) * 2 - 1) * k
    return dict(w1=r(8, 16, 3, 3, k=144 ** -0.5), b1=r(8, k=144 ** -0.5), g2=1 + r(8, k=0.3), be2=r(8, k=0.3),
                w4=r(1, 8, 3, 3, k=72 ** -0.5), b4=r(1, k=72 ** -0.5), rm2=r(8, k=0.2), rv2=1 + r(8, k=0.3))


def _bn64(x, rm, rv, gamma, beta):
    """training-mode batch_norm in fp64: output, saved mean / biased variance; rm / rv updated in place"""
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=MOM, eps=EPS)
    return y, x.mean(dim=(0, 2, 3)), x.var(dim=(0, 2, 3), unbiased=False)


def encoder_fp64(s, P, da1):
    p = {k: v.double().clone() for k, v in P.items()}
    for k in ("w0", "b0", "g1", "be1", "w4", "b4", "g5", "be5"):
        p[k].requires_grad_(True)
    c0 = F.conv2d(s.double(), p["w0"], p["b0"], padding=1)
    n0, m0, v0 = _bn64(c0, p["rm1"], p["rv1"], p["g1"], p["be1"])
    a0 = F.relu(n0)
    p0 = F.max_pool2d(a0, (1, 4))
    c1 = F.conv2d(p0, p["w4"], p["b4"], padding=1)
    n1, m1, v1 = _bn64(c1, p["rm5"], p["rv5"], p["g5"], p["be5"])
    a1 = F.relu(n1)
    for t in (c0, a0, c1):
        t.retain_grad()
    (a1 * da1.double()).sum().backward()
    fwd = dict(a0=a0, p0=p0, c1=c1, a1=a1, m0=m0, v0=v0, m1=m1, v1=v1, rm1=p["rm1"], rv1=p["rv1"], rm5=p["rm5"], rv5=p["rv5"])
    bwd = dict(dw0=p["w0"].grad, db0=p["b0"].grad, dg1=p["g1"].grad, dbe1=p["be1"].grad, dw4=p["w4"].grad, db4=p["b4"].grad,
               dg5=p["g5"].grad, dbe5=p["be5"].grad, dc1=c1.grad, da0=a0.grad, dc0=c0.grad)
    return {k: v.detach() for k, v in fwd.items()}, bwd, c0.detach()


def _grad_buffers(dev):
    z = lambda *s: torch.zeros(*s, device=dev)
    return dict(dw0=z(8, 1, 3, 3), db0=z(8), dg1=z(8), dbe1=z(8), dw4=z(16, 8, 3, 3), db4=z(16), dg5=z(16), dbe5=z(16))


def encoder_generic(ops, s, P, da1, G):
    """today's chain: 9 launches forward, 10 backward (engine.py's structure encoder, cnn.hip + norm.hip)"""
    c0 = ops.conv3x3_fwd(s, P["w0"], P["b0"], G, 1, 8, 4, 32)
    m0, v0 = ops.bn_stats(c0, G, 8, 128, P["rm1"], P["rv1"], MOM)
    a0 = ops.bn_apply(c0, G, 8, 128, m0, v0, P["g1"], P["be1"], EPS, relu=True)
    p0 = ops.maxpool4_fwd(a0).view(G, 8, 4, 8)
    c1 = ops.conv3x3_fwd(p0, P["w4"], P["b4"], G, 8, 16, 4, 8)
    m1, v1 = ops.bn_stats(c1, G, 16, 32, P["rm5"], P["rv5"], MOM)
    a1 = ops.bn_apply(c1, G, 16, 32, m1, v1, P["g5"], P["be5"], EPS, relu=True)
    fwd = dict(c0=c0, a0=a0, p0=p0, c1=c1, a1=a1, m0=m0, v0=v0, m1=m1, v1=v1, rm1=P["rm1"], rv1=P["rv1"], rm5=P["rm5"], rv5=P["rv5"])
    g = _grad_buffers(s.device)
    dc1 = ops.bn_bwd(c1, da1, G, 16, 32, m1, v1, P["g5"], P["be5"], g["dg5"], g["dbe5"], EPS, relu=True)
    ops.conv3x3_bwd_weight(p0, dc1, G, 8, 16, 4, 8, g["dw4"], g["db4"])
    dp0 = ops.conv3x3_bwd_data(dc1, P["w4"], G, 8, 16, 4, 8)
    da0 = ops.maxpool4_bwd(a0, dp0).view(G, 8, 4, 32)
    dc0 = ops.bn_bwd(c0, da0, G, 8, 128, m0, v0, P["g1"], P["be1"], g["dg1"], g["dbe1"], EPS, relu=True)
    ops.conv3x3_bwd_weight(s, dc0, G, 1, 8, 4, 32, g["dw0"], g["db0"])
    return fwd, dict(g, dc1=dc1, da0=da0, dc0=dc0)


def encoder_fused(ops, s, P, da1, G):
    fwd = ops.cnn_enc_fwd(s, P["w0"], P["b0"], P["g1"], P["be1"], P["w4"], P["b4"], P["g5"], P["be5"], G, P["rm1"], P["rv1"],
                          P["rm5"], P["rv5"], EPS, MOM)
    g = _grad_buffers(s.device)
    dc1, da0, dc0 = ops.cnn_enc_bwd(s, fwd, da1, P["g1"], P["be1"], P["g5"], P["be5"], P["w4"], G, g["dw0"], g["db0"], g["dg1"],
                                    g["dbe1"], g["dw4"], g["db4"], g["dg5"], g["dbe5"], EPS)
    return dict(fwd, rm1=P["rm1"], rv1=P["rv1"], rm5=P["rm5"], rv5=P["rv5"]), dict(g, dc1=dc1, da0=da0, dc0=dc0)


@pytest.fixture(scope="module", params=SIZES, ids=[f"G{g}" for g in SIZES])
def encoder_case(request):
    """inputs, the fp64 reference and both chains' results for one size: computed once, shared by the encoder tests"""
    from polyphemus_amd import ops
    G = request.param
    dev = torch.device("cuda")
    s = structure_grids(G, 100 + G)
    P = encoder_params(7)
    da1 = torch.randn(G, 16, 4, 8, generator=torch.Generator().manual_seed(200 + G))
    ref_fwd, ref_bwd, ref_c0 = encoder_fp64(s, P, da1)
    on = lambda: {k: v.to(dev).contiguous() for k, v in P.items()}
    old = encoder_generic(ops, s.to(dev), on(), da1.to(dev), G)
    new = encoder_fused(ops, s.to(dev), on(), da1.to(dev), G)
    torch.cuda.synchronize()
    return dict(G=G, ref_fwd=ref_fwd, ref_bwd=ref_bwd, ref_c0=ref_c0, old=old, new=new)


def test_encoder_forward(encoder_case):
    e = encoder_case
    (old, _), (new, _) = e["old"], e["new"]
    assert torch.equal(new["c0"], old["c0"])                       # same accumulation order: the same bits
    assert rel_l2(new["c0"], e["ref_c0"]) < 1e-6
    fig = check_factor_two(f"enc_fwd G={e['G']}", new, old, e["ref_fwd"])
    assert all(a < 1e-5 for a, _ in fig.values()), fig            # (and close in absolute terms: a broken reference chain must not pass)


def test_encoder_backward(encoder_case):
    e = encoder_case
    (_, old), (_, new) = e["old"], e["new"]
    fig = check_factor_two(f"enc_bwd G={e['G']}", new, old, e["ref_bwd"])
    # (absolute sanity beside the factor-two rule.  A bias in front of a training-mode norm has no gradient: db0 / db4 are sums
    # of dc0 / dc1, zero in exact arithmetic, the reference holds fp64 rounding noise — they are held to the weight gradient's scale)
    assert all(a < 1e-4 for k, (a, _) in fig.items() if k not in ("db0", "db4")), fig
    for kb, kw in (("db0", "dw0"), ("db4", "dw4")):
        assert float(new[kb].abs().max()) < 1e-5 * float(e["ref_bwd"][kw].abs().max()), kb
    # the pool's backward: gradient lands on torch's positions (first maximum among equal zeros behind the ReLU)
    got, want = new["da0"].cpu() != 0, e["ref_bwd"]["da0"] != 0
    assert torch.equal(got, want), int((got != want).sum())
    assert int(want.sum()) > 0


@pytest.mark.parametrize("G", SIZES)
def test_decoder_forward(G):
    from polyphemus_amd import ops
    dev = torch.device("cuda")
    P = decoder_params(9)
    u2 = torch.relu(torch.randn(G, 16, 4, 8, generator=torch.Generator().manual_seed(300 + G)))    # (behind CNNDecoder.lin's ReLU)
    p = {k: v.double().clone() for k, v in P.items()}
    c2r = F.conv2d(F.interpolate(u2.double(), scale_factor=(1, 4), mode="nearest"), p["w1"], p["b1"], padding=1)
    n2, m2, v2 = _bn64(c2r, p["rm2"], p["rv2"], p["g2"], p["be2"])
    a2r = F.relu(n2)
    ref = dict(a2=a2r, s_logits=F.conv2d(a2r, p["w4"], p["b4"], padding=1), m2=m2, v2=v2, rm2=p["rm2"], rv2=p["rv2"])
    on = lambda: {k: v.to(dev).contiguous() for k, v in P.items()}
    # today's chain: 5 launches
    Q = on()
    c2 = ops.conv3x3_fwd(u2.to(dev), Q["w1"], Q["b1"], G, 16, 8, 4, 32, up4=True)
    mo, vo = ops.bn_stats(c2, G, 8, 128, Q["rm2"], Q["rv2"], MOM)
    a2 = ops.bn_apply(c2, G, 8, 128, mo, vo, Q["g2"], Q["be2"], EPS, relu=True)
    old = dict(a2=a2, s_logits=ops.conv3x3_fwd(a2, Q["w4"], Q["b4"], G, 8, 1, 4, 32), m2=mo, v2=vo, rm2=Q["rm2"], rv2=Q["rv2"])
    R = on()
    new = ops.cnn_dec_fwd(u2.to(dev), R["w1"], R["b1"], R["g2"], R["be2"], R["w4"], R["b4"], G, R["rm2"], R["rv2"], EPS, MOM)
    new = dict(new, rm2=R["rm2"], rv2=R["rv2"])
    assert torch.equal(new["c2"], c2)
    assert rel_l2(c2, c2r) < 1e-6
    fig = check_factor_two(f"dec_fwd G={G}", new, old, ref)
    assert all(a < 1e-5 for a, _ in fig.values()), fig


def test_grid_is_sized_to_the_scratch():
    """Scratches that cap the grids: 200 doubles hold 4 slots of the encoder forward and 12 of the decoder, PM_BN_SCRATCH(16) holds
    9 of the backward, so every kernel walks up to 17 of the 67 bars per workgroup.  Every output against the run with one bar per
    workgroup: the fp32 arithmetic per element is the same, only the association of the fp64 sums differs (1e-5 is two orders
    above what that can move an fp32 result; db0 / db4, zero in exact arithmetic, are held to the weight gradient's scale)."""
    from polyphemus_amd import ops
    dev = torch.device("cuda")
    G = 67
    s, P = structure_grids(G, 167).to(dev), {k: v.to(dev) for k, v in encoder_params(7).items()}
    D = {k: v.to(dev) for k, v in decoder_params(9).items()}
    da1 = torch.randn(G, 16, 4, 8, generator=torch.Generator().manual_seed(267)).to(dev)
    u2 = torch.relu(torch.randn(G, 16, 4, 8, generator=torch.Generator().manual_seed(367))).to(dev)
    small = lambda n: torch.empty(n, dtype=torch.float64, device=dev)
    res = []
    for fwd_scr, bwd_scr in ((small(200), ops.bn_scratch(16, dev)), (None, None)):
        Q = {k: v.clone() for k, v in P.items()}
        fwd = ops.cnn_enc_fwd(s, Q["w0"], Q["b0"], Q["g1"], Q["be1"], Q["w4"], Q["b4"], Q["g5"], Q["be5"], G, Q["rm1"], Q["rv1"],
                              Q["rm5"], Q["rv5"], EPS, MOM, scratch=fwd_scr)
        g = _grad_buffers(dev)
        dc1, da0, dc0 = ops.cnn_enc_bwd(s, fwd, da1, Q["g1"], Q["be1"], Q["g5"], Q["be5"], Q["w4"], G, g["dw0"], g["db0"], g["dg1"],
                                        g["dbe1"], g["dw4"], g["db4"], g["dg5"], g["dbe5"], EPS, scratch=bwd_scr)
        R = {k: v.clone() for k, v in D.items()}
        dec = ops.cnn_dec_fwd(u2, R["w1"], R["b1"], R["g2"], R["be2"], R["w4"], R["b4"], G, R["rm2"], R["rv2"], EPS, MOM, scratch=fwd_scr)
        res.append(dict(fwd, rm1=Q["rm1"], rv1=Q["rv1"], rm5=Q["rm5"], rv5=Q["rv5"], dc1=dc1, da0=da0, dc0=dc0, **g, **dec,
                        rm2=R["rm2"], rv2=R["rv2"]))
    capped, free = res
    assert torch.equal(capped["c0"], free["c0"]) and torch.equal(capped["c2"], free["c2"])
    assert torch.equal(capped["da0"].ne(0), free["da0"].ne(0))
    for k in free:
        if k in ("db0", "db4"):
            assert float((capped[k] - free[k]).abs().max()) < 1e-5 * float(free["dw" + k[2]].abs().max()), k
        else:
            assert rel_l2(capped[k], free[k]) < 1e-5, k


class _switches:
    """step switches for the block: set, re-read by the library, restored"""

    def __init__(self, **env):
        self.env = env

    def _apply(self, values):
        from polyphemus_amd._lib import lib
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        assert lib().pm_vae_step_reload_switches() == 0

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.env}
        self._apply(self.env)

    def __exit__(self, *exc):
        self._apply(self.prev)
        return False


def _step(spec, fused):
    from polyphemus_amd import _lib
    live = {}
    with _switches(PM_CNN_FUSED=int(fused)), _lib.deterministic(True):
        run = hip_fullsize_step(spec, lr=0.0, keep=live)
    run["buffers"] = {k: v.detach().cpu().clone() for k, v in live["vae"].state_dict().items() if "running_" in k}
    return run


def test_step_with_fused_cnn_is_as_close_to_the_fp64_oracle_as_with_the_generic_chain():
    # the smallest spec of tests/util.py (B = 24, 48 bars, d = 128) at the bench's depth: 8 layers per stack = 152 parameter tensors
    spec = dict(min(SMALLSIZE.values(), key=lambda s: s["B"] * s["nb"] * s["d"] * s["L"]), L=8)
    new, again, old = _step(spec, True), _step(spec, True), _step(spec, False)
    names = new["names"]
    assert len(names) == 152
    for n in names:                                                # deterministic mode: the same bits in two runs
        assert torch.equal(new["grads"][n], again["grads"][n]), n
    for k in new["buffers"]:
        assert torch.equal(new["buffers"][k], again["buffers"][k]), k
    assert new["losses"] == again["losses"]
    states = {}
    res, _ = oracle_fullsize(spec, new, dtypes=(("o64", torch.float64),), states=states)
    _, l64, g64 = res["o64"]
    for k in ("pitch", "dur", "structure", "kld"):
        a, b = abs(new["losses"][k] - l64[k]), abs(old["losses"][k] - l64[k])
        print("loss", k, a, b)
        assert a <= 2.0 * b, (k, a, b)
    live = [n for n in names if g64[n] is not None]
    check_factor_two("step grads", {n: new["grads"][n] for n in live}, {n: old["grads"][n] for n in live}, {n: g64[n] for n in live})
    bufs = {f"{k}.{t}": states["o64"][f"{k}.{t}"] for k in bn_keys(states["o64"]) for t in ("running_mean", "running_var")}
    assert sorted(bufs) == sorted(new["buffers"])
    check_factor_two("step buffers", new["buffers"], old["buffers"], bufs)
