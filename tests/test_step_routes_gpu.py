"""Which kernels the native training step launches, per width, density, constructor switch, mode and step switch — recorded
once and compared from then on (tests/golden/step_routes.json; `python tests/test_step_routes_gpu.py` on the GPU box rewrites it).

csrc/vae_step.hip decides on the host which kernels a GCN stack takes (fused GCL kernels, bar-resident aggregation, grouped planes
products, the 7-block product; the fp16 pair format; where the norm backward and the residual ride).  A change that only
re-organises those decisions must leave every row of the table as it is.  The same holds for the chains around the stacks
(chord encoder, chord decoder, un-embedding: the head cases of `_cases`).  Observed per case, on one step of a small batch
(n_bars = 2, L = 2, message dropout 0.1, the default seed of `synthetic_batch`):

    the 40 launch-class counts of the in-library profiler (GEMM classes, both segment-reduce directions, the three GCL kernels,
    the chord products: the launches the route decides), the `step_info()` dict and the workspace bytes: EQUAL to the record;
    the four losses: within 1e-6 * max(1, |loss|) — what one step under two kernel orders agrees to (tests/test_fullsize_gpu.py).

The part without a GPU (unmarked) pins `pm_vae_step_workspace_bytes` — the launch-free pass over the step's own carve-outs — for
the same model configurations and switch rows at two fixed batch shapes: a route decision must never move the arena."""
import ctypes
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

GOLDEN = os.path.join(HERE, "golden", "step_routes.json")

SPARSE = dict(B=8, nb=2, L=2, p=0.25, dense=False, msg_p=0.1, seed=1234)
DENSE = dict(B=4, nb=2, L=2, p=1.0, dense=True, msg_p=0.1, seed=1234)          # 1,024 nodes, 128-node bars
# every live switch of the step at its non-default value (csrc/vae_step.hip read_cfg)
SWITCH_ROWS = [("PM_GCL_FUSED", 0), ("PM_GCL_NO_DW", 1), ("PM_NO_ROWS_W", 1), ("PM_GCL_NO_CLASSES", 1), ("PM_FUSED_CE", 0),
               ("PM_SIDE_STREAM", 0), ("PM_SIDE_DELAY_US", 100), ("PM_DAGG_BN", 0), ("PM_DAGG_RES", 0), ("PM_PLAN_SIDE", 0),
               ("PM_CHORD_TABLES", 0), ("PM_H2", 0), ("PM_BAR_ROUTE", 0), ("PM_PAD_SKIP", 0), ("PM_UNEMBED_DW", 0),
               ("PM_SENC_FIRST", 0), ("PM_GCL_OFFSET_LIMIT", 1 << 20), ("PM_DEBUG", 1)]


def _cases():
    """(id, spec, deterministic, env)"""
    out = [("d32_sparse", dict(SPARSE, d=32), False, {})]
    out += [(f"d{d}_sparse", dict(SPARSE, d=d), False, {}) for d in (128, 256, 512)]
    out += [(f"d{d}_dense", dict(DENSE, d=d), False, {}) for d in (128, 256, 512)]
    out += [("d256_sparse_bn_off", dict(SPARSE, d=256, batch_norm=False), False, {}),
            ("d256_sparse_dropout", dict(SPARSE, d=256, dropout=0.1), False, {}),
            ("d256_sparse_seven_block", dict(SPARSE, d=256, track_unique=False), False, {}),
            ("d256_sparse_det", dict(SPARSE, d=256), True, {}),
            ("d512_dense_det", dict(DENSE, d=512), True, {})]
    out += [(f"d256_sparse_{k}={v}", dict(SPARSE, d=256), False, {k: v}) for k, v in SWITCH_ROWS]
    out += [(f"d512_dense_{k}={v}", dict(DENSE, d=512), False, {k: v}) for k, v in (("PM_BAR_ROUTE", 0), ("PM_H2", 0))]
    # the head's decisions (chord encoder / decoder, un-embedding): the bench's head stores no logits; the structure loss on the
    # logits; the accuracy counts; all 15 slots (the full-width chord products); the chord encoder per width without the tables
    s256 = dict(SPARSE, d=256)
    out += [("d256_sparse_keep_logits_off", dict(s256, keep_logits=False), False, {}),
            ("d256_sparse_keep_logits_off_PM_PAD_SKIP=0", dict(s256, keep_logits=False), False, {"PM_PAD_SKIP": 0}),
            ("d256_sparse_fix_structure", dict(s256, fix_structure=True), False, {}),
            ("d256_sparse_metrics", dict(s256, train_metrics=True), False, {}),
            ("d256_sparse_metrics_PM_FUSED_CE=0", dict(s256, train_metrics=True), False, {"PM_FUSED_CE": 0}),
            ("d256_sparse_all_slots", dict(s256, n_slots=15), False, {}),
            ("d256_sparse_all_slots_PM_CHORD_TABLES=0", dict(s256, n_slots=15), False, {"PM_CHORD_TABLES": 0}),
            ("d512_sparse_PM_CHORD_TABLES=0", dict(SPARSE, d=512), False, {"PM_CHORD_TABLES": 0}),
            ("d128_sparse_PM_CHORD_TABLES=0", dict(SPARSE, d=128), False, {"PM_CHORD_TABLES": 0}),
            ("d256_sparse_dropout_fix_structure", dict(s256, dropout=0.1, fix_structure=True), False, {})]
    return out


CASES = _cases()
# the part without a GPU: (id, model configuration, env) x SHAPES
SHAPES = [(500, 3000, 16, 8, 6), (500, 9000, 16, 8, 15)]            # (N, E, G, B, S)


def _cpu_cases():
    cfg = lambda d, L=2, **kw: dict(dict(dropout=0, batch_norm=True, gnn_n_layers=L, d=d, n_bars=2, resolution=8), **kw)
    out = [(f"d{d}", cfg(d), {}) for d in (32, 128, 256, 512)]
    out += [("d256_L3", cfg(256, 3), {}), ("d256_bn_off", cfg(256, batch_norm=False), {}), ("d256_dropout", cfg(256, dropout=0.1), {})]
    out += [(f"d256_{k}={v}", cfg(256), {k: v}) for k, v in SWITCH_ROWS]
    out += [(f"d512_{k}={v}", cfg(512), {k: v}) for k, v in (("PM_BAR_ROUTE", 0), ("PM_H2", 0))]
    return out


CPU_CASES = _cpu_cases()


class _switches:
    """the step switches of `env` for the block: set, re-read by the library (pm_vae_step_reload_switches), and restored"""

    def __init__(self, env):
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


def observe_step(spec, det, env):
    """one native step of `spec` under `env` (and the deterministic mode): what the record holds of it"""
    from polyphemus_amd import _lib
    from util import hip_fullsize_step
    with _switches(env), _lib.deterministic(det):
        keep = {}
        run = hip_fullsize_step(spec, lr=0.0, keep=keep)
        st = keep["trainer"].step
        bt = st.bt
        nbytes = int(_lib.lib().pm_vae_step_workspace_bytes(ctypes.byref(st.layout), bt.N, bt.E, bt.G, bt.B, bt.n_slots))
        info = keep["trainer"].step_info()
    return dict(counts=run["info"]["launch_counts"], info=info, bytes=nbytes,
                losses={k: float(run["losses"][k]) for k in ("pitch", "dur", "structure", "kld")})


def workspace_bytes(cfg, env):
    """pm_vae_step_workspace_bytes of a model of `cfg` under `env` at SHAPES (host only: no GPU is touched)"""
    from polyphemus_amd import _lib
    from polyphemus_amd.model import VAE
    from polyphemus_amd.native import build_layout
    torch.manual_seed(0)
    lay = build_layout(VAE(**cfg, device=torch.device("cpu")))
    with _switches(env):
        return [int(_lib.lib().pm_vae_step_workspace_bytes(ctypes.byref(lay), *shape)) for shape in SHAPES]


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec,det,env", CASES, ids=[c[0] for c in CASES])
def test_step_takes_the_recorded_route(record, name, spec, det, env):
    want = record["steps"][name]
    got = observe_step(spec, det, env)
    print(name, json.dumps(got))
    assert got["counts"] == want["counts"]
    assert got["info"] == want["info"]
    assert got["bytes"] == want["bytes"]
    for k, v in want["losses"].items():
        assert abs(got["losses"][k] - v) <= 1e-6 * max(1.0, abs(v)), (k, got["losses"][k], v)


@pytest.mark.parametrize("name,cfg,env", CPU_CASES, ids=[c[0] for c in CPU_CASES])
def test_workspace_bytes_are_the_recorded_ones(record, name, cfg, env):
    got = workspace_bytes(cfg, env)
    print(name, got)
    assert got == record["workspace"][name]


def test_record_covers_exactly_the_cases(record):
    assert sorted(record["steps"]) == sorted(c[0] for c in CASES)
    assert sorted(record["workspace"]) == sorted(c[0] for c in CPU_CASES)
    assert record["shapes"] == [list(s) for s in SHAPES]


if __name__ == "__main__":                              # rewrite the record (GPU box; the steps part needs the device)
    out = os.environ.get("STEP_ROUTES_OUT", GOLDEN)
    rec = dict(shapes=[list(s) for s in SHAPES], steps={}, workspace={})
    for name, cfg, env in CPU_CASES:
        rec["workspace"][name] = workspace_bytes(cfg, env)
    for name, spec, det, env in CASES:
        rec["steps"][name] = observe_step(spec, det, env)
        print(name, rec["steps"][name]["info"], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
