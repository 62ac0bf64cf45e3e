"""Checks of infill that need no GPU: pm_infill_structure and pm_infill_tokens are declared in include/polyphemus_hip.h
("Infill", behind "Notes in"), exported by the library and bound in the ctypes table with the header's argument lists, the ABI
version is unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can stand in
for device addresses), the Python surface rejects bad arguments without a device, and the numpy restatement the GPU tests
compare with (tests/infill_util.py) gives back the input for an empty region and the model's draw for a full one."""
import os
import re
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from infill_util import infill_ref
from notes_in_util import notes_ref, tokens_ref
from notes_util import CASES, GOLDEN
from test_abi import HEADER, header_prototypes

SIGS = {"pm_infill_structure": "pppiippps", "pm_infill_tokens": "pppiiplplppps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
S_IN, S_MODEL, REGION, S_F32, S_U8, FORCED, S_OUT, TOK_IN, TOK, SCRATCH, STATUS = (0x10000000 + k * 0x100000 for k in range(11))
G, R, N_IN, N = 6, 2, 40, 46
N_SCRATCH = 6 * G + 2
GOOD_S = dict(s_in=S_IN, s_model=S_MODEL, region=REGION, G=G, R=R, s_f32=S_F32, s_u8=S_U8, bar_forced=FORCED)
GOOD_T = dict(s_in=S_IN, s_out=S_OUT, region=REGION, G=G, R=R, tokens_in=TOK_IN, N_in=N_IN, tokens=TOK, N=N, bar_forced=FORCED,
              scratch=SCRATCH, status=STATUS)


def _structure(**kw):
    return _lib.lib().pm_infill_structure(*{**GOOD_S, **kw}.values(), None)


def _tokens(**kw):
    return _lib.lib().pm_infill_tokens(*{**GOOD_T, **kw}.values(), None)


def test_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in SIGS.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig and len(getattr(L, name).argtypes) == len(sig) and name in _lib.EXPORTED
    src = open(HEADER).read()
    section = src[src.index("------ Infill"):src.index("------ message aggregation")]
    assert src.index("------ Notes in") < src.index("------ Infill") < src.index("int pm_infill_structure") < src.index("int pm_infill_tokens")
    assert "data.py:152-153" in section and "preprocess.py:118-157" in section
    assert re.search(r"#define PM_INFILL_SCRATCH\(G\) \(6 \* \(int64_t\)\(G\) \+ 2\)", section)
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


BAD_S = [dict(s_in=None), dict(s_model=None), dict(region=None), dict(s_f32=None, s_u8=None), dict(bar_forced=None),
         dict(G=0), dict(G=-6), dict(R=0), dict(R=-2), dict(R=4), dict(R=5), dict(R=12), dict(G=7),
         dict(G=1 << 24, R=1), dict(G=1 << 30, R=1 << 30),                                     # 128 G beyond int32
         dict(s_in=S_IN + 2), dict(s_f32=S_F32 + 1), dict(s_f32=S_F32 + 2, s_u8=None), dict(bar_forced=FORCED + 3),
         # an output on an input, on another output; ranges that share their last / first byte
         dict(s_f32=S_IN), dict(s_u8=S_IN + 4 * (128 * G - 1)), dict(bar_forced=S_IN), dict(s_f32=S_MODEL), dict(s_u8=S_MODEL + 128 * G - 1),
         dict(bar_forced=S_MODEL + 4), dict(s_f32=REGION), dict(s_u8=REGION + 128 * R - 1), dict(bar_forced=REGION + 128 * R - 4),
         dict(s_u8=S_F32), dict(s_u8=S_F32 + 4 * 128 * G - 1), dict(bar_forced=S_F32 + 4 * (128 * G - 1)), dict(bar_forced=S_U8),
         dict(s_f32=FORCED + 4 * (G - 1)), dict(s_f32=None, s_u8=S_MODEL), dict(s_u8=None, s_f32=S_IN)]
BAD_T = [dict(s_in=None), dict(s_out=None), dict(region=None), dict(tokens_in=None), dict(tokens=None), dict(scratch=None),
         dict(status=None), dict(G=0), dict(G=-1), dict(R=0), dict(R=-3), dict(R=4), dict(R=12), dict(G=7),
         dict(N=-1), dict(N_in=-1), dict(N=-(1 << 40)), dict(N_in=-(1 << 40)),
         # sizes beyond 32 bits: 128 G, 30 N, 32 N_in
         dict(G=1 << 24, R=1), dict(N=1 << 27), dict(N=1 << 62), dict(N_in=1 << 26), dict(N_in=1 << 62),
         # misaligned: 4 bytes, 8 for the tokens, 16 for the input's tokens
         dict(s_in=S_IN + 2), dict(s_out=S_OUT + 1), dict(bar_forced=FORCED + 2), dict(scratch=SCRATCH + 3), dict(status=STATUS + 2),
         dict(tokens=TOK + 4), dict(tokens=TOK + 2), dict(tokens_in=TOK_IN + 8), dict(tokens_in=TOK_IN + 4),
         # the tokens, the scratch and the status on every input and on each other
         dict(tokens=S_IN), dict(tokens=S_OUT + 4 * (128 * G - 2)), dict(tokens=REGION + 8 * (16 * R - 1)), dict(tokens=TOK_IN),
         dict(tokens=TOK_IN + 8 * (16 * N_IN - 1)), dict(tokens=FORCED), dict(tokens_in=TOK + 16 * (15 * N // 2 - 1)),
         dict(scratch=S_IN), dict(scratch=S_OUT), dict(scratch=REGION + 128 * R - 4), dict(scratch=TOK_IN), dict(scratch=FORCED + 4 * (G - 1)),
         dict(status=S_IN + 4 * (128 * G - 1)), dict(status=S_OUT), dict(status=REGION), dict(status=TOK_IN + 4 * (32 * N_IN - 1)), dict(status=FORCED),
         dict(scratch=TOK), dict(scratch=TOK + 4 * (30 * N - 1)), dict(status=TOK), dict(status=TOK + 4 * (30 * N - 1)),
         dict(status=SCRATCH), dict(status=SCRATCH + 4 * (N_SCRATCH - 1)), dict(scratch=STATUS + 4 * 4), dict(tokens=STATUS + 8)]
_ids = lambda d: "-".join(f"{k}={v}" for k, v in d.items())


@pytest.mark.parametrize("bad", BAD_S, ids=_ids)
def test_infill_structure_rejects_on_the_host(bad):
    assert _structure(**bad) == PM_E_INVALID


@pytest.mark.parametrize("bad", BAD_T, ids=_ids)
def test_infill_tokens_rejects_on_the_host(bad):
    assert _tokens(**bad) == PM_E_INVALID


def test_no_nodes_still_check_everything_else():
    """N_in == 0: tokens_in may be NULL; N == 0: tokens may be NULL; the other arguments are checked as ever"""
    for kw in (dict(N_in=0, tokens_in=None), dict(N=0, tokens=None), dict(N_in=0, tokens_in=None, N=0, tokens=None)):
        assert _tokens(**kw, status=None) == PM_E_INVALID
        assert _tokens(**kw, R=4) == PM_E_INVALID
        assert _tokens(**kw, status=SCRATCH) == PM_E_INVALID
        assert _tokens(**kw, s_out=S_OUT + 2) == PM_E_INVALID


def test_region_mask_values():
    from polyphemus_amd.generate import TRACKS, region_mask, step_mask
    full = region_mask(3)
    assert full.dtype == np.bool_ and full.shape == (3, 4, 32) and full.all() and full.flags["C_CONTIGUOUS"]
    g = region_mask(2, tracks=["Guitar"])
    assert g[:, 2].all() and g.sum() == 64 and np.array_equal(g, region_mask(2, tracks=(2,)))
    gs = region_mask(2, tracks=["Guitar", "Strings"])
    assert gs[:, 2:].all() and not gs[:, :2].any() and np.array_equal(gs, region_mask(2, tracks=[TRACKS.index("Strings"), "Guitar"]))
    b = region_mask(3, bars=[1])
    assert b[1].all() and b.sum() == 128
    w = region_mask(2, steps=step_mask(lo=8, hi=15))
    assert w[:, :, 8:16].all() and w.sum() == 2 * 4 * 8
    every = region_mask(2, tracks=["Bass"], bars=[0], steps=step_mask(every=4))
    assert every.sum() == 8 and every[0, 1, ::4].all()
    assert not region_mask(2, tracks=[]).any() and not region_mask(2, bars=[]).any()
    for kw, name in ((dict(tracks=["Piano"]), "tracks"), (dict(tracks=[4]), "tracks"), (dict(tracks="Guitar"), "tracks"), (dict(tracks=[1.0]), "tracks"),
                     (dict(tracks=[True]), "tracks"), (dict(bars=[2]), "bars"), (dict(bars=[-1]), "bars"), (dict(bars=1), "bars"),
                     (dict(bars=[0.0]), "bars"), (dict(steps=np.ones(31, bool)), "steps"), (dict(steps=np.ones(32, np.int32)), "steps"),
                     (dict(steps=np.ones((1, 32), bool)), "steps")):
        with pytest.raises(ValueError, match=name):
            region_mask(2, **kw)
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_bars"):
            region_mask(bad)


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import NoteBatch, StructureRules, infill_notes, region_mask
    B, n_bars = 2, 3
    ok = np.zeros((n_bars, 4, 32), bool)
    for good in (ok, ok.tolist(), torch.from_numpy(ok), np.zeros((B, n_bars, 4, 32), bool), ok[:, ::-1]):
        got = ops.check_region(good, B, n_bars)
        assert isinstance(got, np.ndarray) and got.dtype == np.bool_ and got.flags["C_CONTIGUOUS"] and got.shape[-3:] == (n_bars, 4, 32)
    for bad in (ok.astype(np.uint8), ok.astype(np.float32), torch.zeros(n_bars, 4, 32), torch.zeros(n_bars, 4, 32, dtype=torch.uint8),
                ok[:2], ok[:, :3], ok[..., :31], ok.reshape(-1), np.zeros((B + 1, n_bars, 4, 32), bool), np.zeros((1, B, n_bars, 4, 32), bool),
                None, "all", 1, [[True]]):
        with pytest.raises(ValueError, match="region"):
            ops.check_region(bad, B, n_bars)
    # the device wrappers: dtype / shape errors first, then the device
    s, u = torch.zeros(6, 4, 32), torch.zeros(6, 4, 32, dtype=torch.uint8)
    tin, tok, reg = torch.zeros(5, 16, 2, dtype=torch.int32), torch.zeros(7, 15, 2, dtype=torch.int32), torch.zeros(3, 4, 32, dtype=torch.bool)
    for a, b, r, name in ((u, u, reg, "s_in"), (s.double(), u, reg, "s_in"), (s[:, :3], u, reg, "s_in"), (s, s, reg, "s_model"), (s, u[:5], reg, "s_model"),
                          (s, u, reg.float(), "region"), (s, u, reg[:, :, :5], "region"), (s, u, torch.zeros(4, 4, 32, dtype=torch.bool), "region"),
                          (s.numpy(), u, reg, "s_in")):
        with pytest.raises(ValueError, match=name):
            ops.infill_structure(a, b, r)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.infill_structure(s, u, reg)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.infill_structure(s, u.bool(), reg.numpy())
    good = dict(s_in=s, s_out=s, region=reg, tokens_in=tin, tokens=tok)
    for kw, name in ((dict(s_in=u), "s_in"), (dict(s_out=s[:5]), "s_out"), (dict(s_out=s.half()), "s_out"), (dict(tokens_in=tin.long()), "tokens_in"),
                     (dict(tokens_in=tok), "tokens_in"), (dict(tokens_in=tin.reshape(-1, 2)), "tokens_in"), (dict(tokens=tin), "tokens"),
                     (dict(tokens=tok.float()), "tokens"), (dict(tokens=tok[::2]), "tokens"), (dict(tokens=None), "tokens"),
                     (dict(region=reg.int()), "region"), (dict(region=reg[:, :2]), "region"), (dict(bar_forced=torch.zeros(6)), "bar_forced"),
                     (dict(bar_forced=torch.zeros(6, 1, dtype=torch.int32)), "bar_forced")):
        with pytest.raises(ValueError, match=name):
            ops.infill_tokens(**{**good, **kw})
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.infill_tokens(**good)
    # infill_notes: before the model is touched
    nb = NoteBatch.from_lists([[[(0, 60, 4)], [], [(5, 41, 2)], []]] * B, n_bars, device="cpu")
    vae = types.SimpleNamespace(cfg={"n_bars": n_bars})
    with pytest.raises(ValueError, match="NoteBatch"):
        infill_notes(vae, (nb.notes, nb.track_ptr), ok)
    with pytest.raises(ValueError, match=f"n_bars = {n_bars}"):
        infill_notes(types.SimpleNamespace(cfg={"n_bars": n_bars + 1}), nb, ok)
    for bad in (ok.astype(np.uint8), ok[:2], np.zeros((B + 1, n_bars, 4, 32), bool), torch.zeros(n_bars, 4, 32), None, region_mask(n_bars + 1)):
        with pytest.raises(ValueError, match="region"):
            infill_notes(vae, nb, bad)
    for kw, name in ((dict(strength=-0.5), "strength"), (dict(strength=float("inf")), "strength"), (dict(strength=float("nan")), "strength"),
                     (dict(strength="1"), "strength"), (dict(seed=-1), "seed"), (dict(seed=1 << 32), "seed"), (dict(seed=1.5), "seed"),
                     (dict(s_cond=3), "s_cond"), (dict(s_tensor_cond=3), "s_tensor_cond"),
                     (dict(keep_structure=True, structure_rules=StructureRules()), "structure_rules draws the structure itself")):
        with pytest.raises(ValueError, match=name):
            infill_notes(None, None, None, **kw)
    # generate_notes' own checks, still before the model is touched
    for kw, name in ((dict(temperature=-1.0), "temperature"), (dict(top_k=0), "top_k"), (dict(top_p=1.5), "top_p"),
                     (dict(chord_rules=3), "chord_rules"), (dict(structure_rules=3), "structure_rules")):
        with pytest.raises(ValueError, match=name):
            infill_notes(vae, nb, ok, **kw)
    with pytest.raises(TypeError, match="no_such_argument"):
        infill_notes(vae, nb, ok, no_such_argument=1)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        infill_notes(vae, nb, ok)


def _golden_input(name="lmd2_tiny"):
    n_bars = CASES[name][1]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    notes, ptr = notes_ref(z["in/tokens"].astype(np.int32)[:, 1:], z["in/s_tensor"].reshape(-1, n_bars, 4, 32))
    s_in, tokens_in, _ = tokens_ref(notes, ptr, n_bars)
    return s_in, tokens_in, n_bars


def test_restatement_on_a_golden_case_returns_the_input_or_the_draw():
    s_in, tokens_in, n_bars = _golden_input()
    G, N_in = len(s_in), len(tokens_in)
    rng = np.random.default_rng(4)
    s_model = rng.random((G, 4, 32)) < 0.2
    s_model[~s_model.any(axis=(1, 2)), 1, 3] = True
    for shape in ((n_bars, 4, 32), (G, 4, 32), (G // n_bars, n_bars, 4, 32)):
        # region all-False: the input's structure and tokens[:, 1:], whatever was drawn
        drawn = rng.integers(0, 96, (N_in, 15, 2)).astype(np.int32)
        s_out, forced, tokens, status = infill_ref(s_in, tokens_in, s_model, drawn, np.zeros(shape, bool))
        assert s_out.dtype == np.bool_ and np.array_equal(s_out, s_in != 0) and not forced.any() and forced.dtype == np.int32
        assert tokens.dtype == np.int32 and np.array_equal(tokens, tokens_in[:, 1:]) and status.tolist() == [N_in, N_in, N_in, 0, 0]
        # region all-True: the model's structure and the drawn tokens
        N = int(s_model.sum())
        drawn = rng.integers(0, 96, (N, 15, 2)).astype(np.int32)
        s_out, forced, tokens, status = infill_ref(s_in, tokens_in, s_model, drawn, np.ones(shape, bool))
        assert np.array_equal(s_out, s_model) and not forced.any() and np.array_equal(tokens, drawn)
        assert status.tolist() == [N, N_in, 0, 0, 0]
    # one track regenerated: the other tracks' nodes come back in the merged numbering, the track's own stay as drawn
    region = np.zeros((n_bars, 4, 32), bool)
    region[:, 2] = True
    s_out, forced, _, _ = infill_ref(s_in, tokens_in, s_model, np.zeros((0, 15, 2)), region)
    drawn = rng.integers(0, 96, (int(s_out.sum()), 15, 2)).astype(np.int32)
    s_out, forced, tokens, status = infill_ref(s_in, tokens_in, s_model, drawn, region)
    track = np.nonzero(s_out)[1]
    assert np.array_equal(tokens[track == 2], drawn[track == 2])
    assert np.array_equal(tokens[track != 2], tokens_in[np.nonzero(s_in)[1] != 2][:, 1:]) and status[2] == (track != 2).sum() and status[3] == 0
    # a bar that comes out empty: [0,0] forced, outside the region, without a source
    s_one = np.zeros((2, 4, 32), np.float32)
    s_one[0, 3, 7] = s_one[1, 1, 1] = 1
    tok_one = np.tile(np.asarray([[128, 96], [60, 3], [129, 97]] + [[130, 98]] * 13, np.int32), (2, 1, 1))
    region = np.zeros((1, 4, 32), bool)
    region[0, 3] = True
    s_out, forced, tokens, status = infill_ref(s_one, tok_one, np.zeros((2, 4, 32), np.uint8), np.full((2, 15, 2), 5), region)
    assert forced.tolist() == [1, 0] and s_out.sum() == 2 and s_out[0, 0, 0] and s_out[1, 1, 1]
    assert tokens[0].tolist() == [[129, 97]] + [[130, 98]] * 14 and np.array_equal(tokens[1], tok_one[1, 1:])
    assert status.tolist() == [2, 2, 2, 1, 1]
