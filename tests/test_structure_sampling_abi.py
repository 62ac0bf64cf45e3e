"""Checks of structure sampling that need no GPU: the entry is declared in include/polyphemus_hip.h, exported by the library and
bound in the ctypes table with the header's argument list, the ABI version is unchanged, the ctypes mirror of PmStructureRules
has the header's layout, every argument check answers PM_E_INVALID on the host before any launch (so host integers can stand
in for device addresses, next to a real host PmStructureRules), `ops.check_structure_args` and `generate_music` reject bad
values by name before the model is touched, `step_mask` equals hand-written rows, and the noise stream of head 2 is the
numpy hash."""
import ctypes
import re

import numpy as np
import pytest

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes
from test_sampling_abi import sample_hash_np

PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
LOGITS, S_F32, S_U8, COUNT = (0x10000000 + k * 0x100000 for k in range(4))
NAN, INF = float("nan"), float("inf")
FULL = 0xFFFFFFFF


def _rules(temperature=1.0, bias=(0.0,) * 4, min_active=(0,) * 4, max_active=(32,) * 4, step_mask=(FULL,) * 4):
    r = _lib.PmStructureRules()
    r.temperature = temperature
    for k in range(4):
        r.bias[k], r.min_active[k], r.max_active[k], r.step_mask[k] = bias[k], min_active[k], max_active[k], step_mask[k]
    return r


def _sample(s_logits=LOGITS, G=3, rules="default", s_f32=S_F32, s_u8=S_U8, track_count=COUNT, **kw):
    r = _rules(**kw) if rules == "default" else rules
    return _lib.lib().pm_sample_structure(s_logits, G, None if r is None else ctypes.addressof(r), 0, s_f32, s_u8, track_count, None)


def test_structure_entry_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    name, sig = "pm_sample_structure", "pipuppps"
    assert protos.get(name) == sig, protos.get(name)
    assert hasattr(L, name), f"{name} not exported"
    assert _lib._SIGS.get(name) == sig, _lib._SIGS.get(name)
    assert len(getattr(L, name).argtypes) == len(sig)
    assert name in _lib.EXPORTED
    src = open(HEADER).read()
    assert re.search(r"typedef struct PmStructureRules \{", src) and "Structure sampling" in src
    assert src.index("Chord-aware sampling") < src.index("Structure sampling.") < src.index("typedef struct PmStructureRules")
    assert "not bit-identical" in src                     # the header does not claim the thresholded rule bit for bit
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


def test_structure_rules_mirror_has_the_header_layout():
    R = _lib.PmStructureRules
    assert ctypes.sizeof(R) == 68
    names = ["temperature", "bias", "min_active", "max_active", "step_mask"]
    assert [getattr(R, f).offset for f in names] == [0, 4, 20, 36, 52]
    assert [n for n, _ in R._fields_] == names
    body = re.search(r"typedef struct PmStructureRules \{(.*?)\} PmStructureRules;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    members = re.findall(r"(float|int32_t|uint32_t)\s+(\w+)((?:\[\d+\])*)\s*;", body)
    assert members == [("float", "temperature", ""), ("float", "bias", "[4]"), ("int32_t", "min_active", "[4]"),
                       ("int32_t", "max_active", "[4]"), ("uint32_t", "step_mask", "[4]")]


BAD_C = [dict(s_logits=None), dict(rules=None), dict(s_f32=None, s_u8=None), dict(G=0), dict(G=-3), dict(G=-(1 << 31)),
         dict(temperature=-1.0), dict(temperature=-1e-30), dict(temperature=NAN), dict(temperature=INF),
         dict(bias=(0.0, NAN, 0.0, 0.0)), dict(bias=(INF, 0.0, 0.0, 0.0)), dict(bias=(0.0, 0.0, 0.0, -INF)),
         dict(min_active=(0, -1, 0, 0)), dict(max_active=(32, 32, 33, 32)), dict(max_active=(32, 32, 32, 1 << 20)),
         dict(min_active=(0, 0, 5, 0), max_active=(32, 32, 4, 32)), dict(max_active=(-1, 32, 32, 32)),
         dict(min_active=(0, 5, 0, 0), step_mask=(FULL, 0x0000000F, FULL, FULL)),
         dict(min_active=(1, 0, 0, 0), step_mask=(0, FULL, FULL, FULL)),
         dict(min_active=(0, 0, 0, 5), max_active=(32, 32, 32, 5), step_mask=(FULL, FULL, FULL, 0x01010101)),
         dict(max_active=(0, 0, 0, 0)), dict(step_mask=(0, 0, 0, 0)),
         dict(max_active=(0, 3, 0, 0), step_mask=(FULL, 0, FULL, FULL)),
         dict(max_active=(0, 0, 8, 8), step_mask=(FULL, FULL, 0, 0))]


@pytest.mark.parametrize("bad", BAD_C, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_sample_structure_rejects_on_the_host(bad):
    assert _sample(**bad) == PM_E_INVALID
    if "temperature" not in bad and "rules" not in bad:
        assert _sample(**{**bad, "temperature": 0.0}) == PM_E_INVALID                 # the route without noise too
    if "s_f32" not in bad:
        for out in (dict(s_f32=None), dict(s_u8=None), dict(track_count=None)):      # each may be NULL alone: not the cause
            assert _sample(**{**bad, **out}) == PM_E_INVALID


ALL = np.ones((4, 32), bool)
EVEN = np.arange(32) % 2 == 0
BAD = [("temperature", v) for v in (-1.0, -1e-9, NAN, INF, -INF, True, "1.0", [1.0], (1.0, 1.0), None)] + \
      [("threshold", v) for v in (0, 0.0, 1, 1.0, -0.1, 1.5, NAN, True, "0.5", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5, 0.5, 0.5),
                                  (0.5, 0.0, 0.5, 0.5), (0.5, 0.5, 1.0, 0.5), (0.5, 0.5, 0.5, NAN), (0.5, True, 0.5, 0.5),
                                  None)] + \
      [("seed", v) for v in (-1, 1 << 32, 1.0, True)] + \
      [("min_active", v) for v in (-1, 33, 1.0, True, "1", (1, 1, 1), (1, 1, 1, 1, 1), (1, 1, -1, 1), (1, 1, 1, 1.5), None)] + \
      [("max_active", v) for v in (-1, 33, 2.0, True, "32", (32, 32, 32), (32, 32, -1, 32), (32, 33, 32, 32), 0, (0, 0, 0, 0),
                                   None)] + \
      [("allowed_steps", v) for v in (np.ones((4, 31), bool), np.ones((3, 32), bool), np.ones(32, bool), np.ones((4, 32), np.float32),
                                      np.ones((4, 32), np.int64), "all", np.zeros((4, 32), bool))]


@pytest.mark.parametrize("name,value", BAD, ids=[f"{n}={np.shape(v) if isinstance(v, np.ndarray) else v!r}" for n, v in BAD])
def test_check_structure_args_and_generate_music_reject_bad_values_by_name(name, value):
    """Before the model (None here) is touched, naming the argument."""
    from polyphemus_amd import ops
    from polyphemus_amd.generate import ChordRules, StructureRules, generate_music
    with pytest.raises(ValueError, match=name):
        ops.check_structure_args(**{name: value})
    if name != "seed":
        with pytest.raises(ValueError, match=name):
            ops.sample_structure(None, **{name: value})              # ... and before the tensor is looked at
    rules = StructureRules() if name == "seed" else StructureRules(**{name: value})
    kw = {name: value} if name == "seed" else {}
    for more in (dict(), dict(temperature=0.8, top_k=5, return_tokens=True), dict(chord_rules=ChordRules(), return_note_counts=True)):
        with pytest.raises(ValueError, match=name):
            generate_music(None, None, structure_rules=rules, **kw, **more)


def test_rules_that_contradict_each_other_are_rejected():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import ChordRules, StructureRules, generate_music
    a = ALL.copy()
    a[1] = np.arange(32) % 8 == 0
    for kw, name in ((dict(min_active=5, max_active=4), "min_active"),
                     (dict(min_active=(0, 0, 7, 0), max_active=(32, 32, 6, 32)), "min_active"),
                     (dict(min_active=(0, 5, 0, 0), allowed_steps=a), "min_active"),                      # 4 allowed steps
                     (dict(max_active=(0, 3, 0, 0), allowed_steps=np.stack([EVEN, ~ALL[0], EVEN, EVEN])), "max_active"),
                     (dict(max_active=(0, 0, 0, 0)), "max_active")):
        with pytest.raises(ValueError, match=name):
            ops.check_structure_args(**kw)
        with pytest.raises(ValueError, match=name):
            generate_music(None, None, structure_rules=StructureRules(**kw))
    ops.check_structure_args(min_active=(0, 4, 0, 0), allowed_steps=a)                                    # exactly the allowed steps
    # the structure is either given or drawn; the keyword takes a StructureRules
    with pytest.raises(ValueError, match="s_cond"):
        generate_music(None, None, object(), structure_rules=StructureRules())
    with pytest.raises(ValueError, match="s_tensor_cond"):
        generate_music(None, None, None, np.zeros((1, 2, 4, 32), bool), structure_rules=StructureRules())
    with pytest.raises(ValueError, match="s_cond"):
        generate_music(None, None, object(), object(), structure_rules=StructureRules(), chord_rules=ChordRules(), seed=3)
    for bad in (dict(min_active=1), ChordRules(), "default", 1.0):
        with pytest.raises(ValueError, match="structure_rules"):
            generate_music(None, None, structure_rules=bad)
    # the content arguments are still checked before the model, with structure rules that are fine
    with pytest.raises(ValueError, match="top_p"):
        generate_music(None, None, structure_rules=StructureRules(), top_p=0.0)
    with pytest.raises(ValueError, match="max_notes"):
        generate_music(None, None, structure_rules=StructureRules(), chord_rules=ChordRules(max_notes=15))
    with pytest.raises(ValueError, match="return_note_counts"):
        generate_music(None, None, structure_rules=StructureRules(), return_note_counts=True)


def test_structure_arguments_that_are_fine():
    import math
    import torch
    from polyphemus_amd import ops
    from polyphemus_amd.generate import StructureRules
    for kw in (dict(), dict(temperature=0), dict(temperature=np.float32(2)), dict(temperature=1e-30), dict(threshold=0.01),
               dict(threshold=(0.5, 0.3, 0.7, 0.999)), dict(threshold=[0.1, 0.2, 0.3, 0.4]), dict(threshold=np.float32(0.25)),
               dict(seed=(1 << 32) - 1), dict(seed=0), dict(min_active=32), dict(min_active=(0, 1, 2, 32)), dict(max_active=(0, 0, 0, 1)),
               dict(max_active=np.int64(3)), dict(max_active=[1, 2, 3, 4], min_active=1), dict(allowed_steps=ALL),
               dict(allowed_steps=ALL.tolist()), dict(allowed_steps=torch.ones(4, 32, dtype=torch.bool)),
               dict(max_active=(0, 2, 0, 1), allowed_steps=np.stack([~ALL[0], EVEN, ~ALL[0], EVEN]))):
        ops.check_structure_args(**kw)
    T, bias, mn, mx, words = ops.check_structure_args(0.5, (0.5, 0.3, 0.7, 0.5), (2, 0, 1, 4), (8, 16, 3, 4))
    assert T == 0.5 and mn == (2, 0, 1, 4) and mx == (8, 16, 3, 4) and words == [FULL] * 4
    assert bias[0] == 0.0 == bias[3] and bias[1] == math.log(0.3 / 0.7) and bias[2] == math.log(0.7 / (1.0 - 0.7))
    a = np.zeros((4, 32), bool)
    a[0, 0] = a[1, 31] = a[2, 1] = a[2, 30] = a[3, 5] = a[3, 16] = True
    words = ops.check_structure_args(max_active=2, allowed_steps=a)[4]
    assert words == [1, 1 << 31, (1 << 1) | (1 << 30), (1 << 5) | (1 << 16)]
    for k in range(4):                                            # the header's rule: bit t of step_mask[k]
        assert [t for t in range(32) if (words[k] >> t) & 1] == list(np.flatnonzero(a[k]))
    r = StructureRules()
    assert (r.temperature, r.threshold, r.min_active, r.max_active, r.allowed_steps) == (1.0, 0.5, 0, 32, None)


def test_step_mask_equals_hand_written_rows():
    from polyphemus_amd.generate import step_mask
    row = lambda *on: np.isin(np.arange(32), on)
    assert step_mask().dtype == np.bool_ and step_mask().shape == (32,) and step_mask().all()
    assert np.array_equal(step_mask(2), row(*range(0, 32, 2)))
    assert np.array_equal(step_mask(8), row(0, 8, 16, 24))
    assert np.array_equal(step_mask(8, 4), row(4, 12, 20, 28))
    assert np.array_equal(step_mask(4, 2, 8, 23), row(10, 14, 18, 22))
    assert np.array_equal(step_mask(1, 0, 16, 31), row(*range(16, 32)))
    assert np.array_equal(step_mask(3, 1), row(*range(1, 32, 3)))
    assert np.array_equal(step_mask(32, 31), row(31)) and np.array_equal(step_mask(5, 0, 5, 5), row(5))
    assert np.array_equal(step_mask(lo=3, hi=3), row(3)) and np.array_equal(step_mask(16, 0, 1, 31), row(16))
    assert not step_mask(lo=9, hi=8).any() and not step_mask(4, 1, 2, 4).any() and not step_mask(1, 32).any()
    with pytest.raises(ValueError, match="every"):
        step_mask(0)


def test_structure_noise_stream_is_head_two_of_the_sampling_hash():
    L = _lib.lib()
    rng = np.random.default_rng(5)
    seeds = [0, 1, 0xFFFFFFFF] + [int(v) for v in rng.integers(0, 1 << 32, 3)]
    bars = [0, 1, 2, 514, (1 << 31) - 1] + [int(v) for v in rng.integers(0, 1 << 31, 2)]
    cells = np.arange(128, dtype=np.uint64)
    for seed in seeds:
        for g in bars:
            want = sample_hash_np(seed, g, 2, cells)
            got = np.array([L.pm_sample_hash(seed, g, 2, int(c)) for c in cells], dtype=np.uint64)
            assert np.array_equal(got, want), (seed, g)
            assert int(want.max()) < 1 << 23
    # head 2 is a stream of its own: the same (seed, row, token) under the pitch and the duration head gives other words
    for head in (0, 1):
        other = sample_hash_np(7, 3, head, cells)
        assert (other != sample_hash_np(7, 3, 2, cells)).mean() > 0.99
