"""Checks of chord-aware sampling that need no GPU: its two entries are declared in include/polyphemus_hip.h, exported by the
library and bound in the ctypes table with the header's argument lists, the ABI version is unchanged, the ctypes mirror of
PmChordRules has the header's layout, every argument check answers PM_E_INVALID on the host before any launch (so host
integers can stand in for device addresses, next to a real host PmChordRules), `ops.check_chord_args` and `generate_music`
reject bad values by name before the model is touched, and `pitch_mask` equals its numpy expression."""
import ctypes
import re

import numpy as np
import pytest

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes

ENTRIES = {"pm_sample_chords": "pplpupps", "pm_node_tracks": "pilppps"}
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
LOGITS, TRACK, TOKENS, COUNT, S, BARS, PTR = (0x10000000 + k * 0x100000 for k in range(7))
NAN, INF = float("nan"), float("inf")


def _rules(temperature=(1.0, 1.0), top_k=0, top_p=1.0, min_notes=(1, 1, 1, 1), max_notes=(14, 14, 14, 14)):
    r = _lib.PmChordRules()
    r.temperature[0], r.temperature[1] = temperature
    r.top_k, r.top_p = top_k, top_p
    for k in range(4):
        r.min_notes[k], r.max_notes[k] = min_notes[k], max_notes[k]
        for w in range(4):
            r.pitch_mask[k][w] = 0xFFFFFFFF
    return r


def _chords(c_logits=LOGITS, node_track=TRACK, N=3, rules="default", tokens=TOKENS, note_count=COUNT, **kw):
    r = _rules(**kw) if rules == "default" else rules
    return _lib.lib().pm_sample_chords(c_logits, node_track, N, None if r is None else ctypes.addressof(r), 0, tokens,
                                       note_count, None)


def _tracks(s=S, G=2, N=7, bars=BARS, ptr=PTR, track=TRACK):
    return _lib.lib().pm_node_tracks(s, G, N, bars, ptr, track, None)


def test_chord_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)
        assert name in _lib.EXPORTED
    src = open(HEADER).read()
    assert re.search(r"typedef struct PmChordRules \{", src) and "Chord-aware sampling" in src
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


def test_chord_rules_mirror_has_the_header_layout():
    R = _lib.PmChordRules
    assert ctypes.sizeof(R) == 112
    offsets = [getattr(R, f).offset for f in ("temperature", "top_k", "top_p", "min_notes", "max_notes", "pitch_mask")]
    assert offsets == [0, 8, 12, 16, 32, 48]
    assert [n for n, _ in R._fields_] == ["temperature", "top_k", "top_p", "min_notes", "max_notes", "pitch_mask"]
    assert R.pitch_mask.size == 64 and R.temperature.size == 8
    # the header's member list, in order, with the same element types and counts
    body = re.search(r"typedef struct PmChordRules \{(.*?)\} PmChordRules;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    members = re.findall(r"(float|int32_t|uint32_t)\s+(\w+)((?:\[\d+\])*)\s*;", body)
    assert [(t, n, d) for t, n, d in members] == [("float", "temperature", "[2]"), ("int32_t", "top_k", ""), ("float", "top_p", ""),
                                                  ("int32_t", "min_notes", "[4]"), ("int32_t", "max_notes", "[4]"),
                                                  ("uint32_t", "pitch_mask", "[4][4]")]


BAD_C = [dict(c_logits=None), dict(node_track=None), dict(rules=None), dict(tokens=None), dict(N=0), dict(N=-3),
         dict(N=(1 << 32) // 15 + 1), dict(N=1 << 40), dict(temperature=(-1.0, 1.0)), dict(temperature=(1.0, -1e-30)),
         dict(temperature=(NAN, 1.0)), dict(temperature=(1.0, NAN)), dict(temperature=(INF, 1.0)), dict(temperature=(0.0, INF)),
         dict(top_k=-1), dict(top_k=-(1 << 31)), dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0000001), dict(top_p=2.0),
         dict(top_p=NAN), dict(top_p=INF), dict(min_notes=(1, -1, 1, 1)), dict(max_notes=(14, 14, 0, 14)),
         dict(max_notes=(14, 14, 14, 15)), dict(max_notes=(-2, 14, 14, 14), min_notes=(0, 1, 1, 1)),
         dict(min_notes=(1, 1, 1, 5), max_notes=(14, 14, 14, 4))]


@pytest.mark.parametrize("bad", BAD_C, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_sample_chords_rejects_on_the_host(bad):
    assert _chords(**bad) == PM_E_INVALID
    if "temperature" not in bad and "rules" not in bad:
        assert _chords(**{**bad, "temperature": (0.0, 0.0)}) == PM_E_INVALID                      # the greedy route too
        assert _chords(**{**dict(top_k=5, top_p=0.9), **bad}) == PM_E_INVALID                    # ... and the filtered one
    assert _chords(**{**bad, "note_count": None}) == PM_E_INVALID                                # note_count may be NULL: not the cause


def test_sample_chords_largest_node_count_is_below_two_to_the_32_rows():
    assert ((1 << 32) // 15) * 15 < 1 << 32 <= ((1 << 32) // 15 + 1) * 15
    assert _chords(N=(1 << 32) // 15 + 1) == PM_E_INVALID


@pytest.mark.parametrize("bad", [dict(track=None), dict(s=None), dict(bars=None), dict(ptr=None), dict(G=0), dict(G=-1),
                                 dict(N=-1), dict(ptr=BARS), dict(G=1 << 29)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_node_tracks_rejects_what_mtp_from_tokens_rejects(bad):
    assert _tracks(**bad) == PM_E_INVALID
    if "track" not in bad:
        names = dict(bars="bar_nodes", ptr="node_ptr", s="s_tensor")
        args = dict(tokens=TOKENS, s_tensor=S, G=2, N=7, bar_nodes=BARS, node_ptr=PTR, mtp=LOGITS)
        args.update({names.get(k, k): v for k, v in bad.items()})
        assert _lib.lib().pm_mtp_from_tokens(*args.values(), None) == PM_E_INVALID


ALL = np.ones((4, 128), bool)
BAD = [("temperature", v) for v in (-1.0, -1e-9, NAN, INF, -INF, True, "1.0", [1.0], (1.0, -1.0), (1.0, NAN), (1.0, 1.0, 1.0),
                                    (1.0, True), (INF, 0.0))] + \
      [("top_k", v) for v in (0, -1, 1.5, True, "5")] + \
      [("top_p", v) for v in (0, 0.0, -0.1, 1.0000001, 2, NAN, True, "0.9")] + \
      [("seed", v) for v in (-1, 1 << 32, 1.0, True)] + \
      [("min_notes", v) for v in (-1, 15, 1.0, True, "1", (1, 1, 1), (1, 1, 1, 1, 1), (1, 1, -1, 1), (1, 1, 1, 1.5))] + \
      [("max_notes", v) for v in (0, 15, -1, 2.0, True, "14", (14, 14, 14), (14, 14, 0, 14), (14, 15, 14, 14))] + \
      [("allowed_pitches", v) for v in (np.ones((4, 127), bool), np.ones((3, 128), bool), np.ones(128, bool),
                                        np.ones((4, 128), np.float32), np.ones((4, 128), np.int64), "all")]


@pytest.mark.parametrize("name,value", BAD, ids=[f"{n}={np.shape(v) if isinstance(v, np.ndarray) else v!r}" for n, v in BAD])
def test_check_chord_args_and_generate_music_reject_bad_values_by_name(name, value):
    """Before the model (None here) is touched, naming the argument."""
    from polyphemus_amd import ops
    from polyphemus_amd.generate import ChordRules, generate_music
    with pytest.raises(ValueError, match=name):
        ops.check_chord_args(**{name: value})
    with pytest.raises(ValueError, match=name):
        ops.check_chord_args(**{**dict(temperature=(1.0, 0.5), top_k=5, top_p=0.9, seed=1, min_notes=1, max_notes=14,
                                       allowed_pitches=ALL), name: value})
    rule_names = ("min_notes", "max_notes", "allowed_pitches")
    rules = ChordRules(**{name: value}) if name in rule_names else ChordRules()
    kw = {} if name in rule_names else {name: value}
    with pytest.raises(ValueError, match=name):
        generate_music(None, None, chord_rules=rules, **kw)
    with pytest.raises(ValueError, match=name):
        generate_music(None, None, chord_rules=rules, return_tokens=True, return_note_counts=True, **{**dict(seed=1), **kw})


def test_min_notes_above_max_notes_is_rejected_and_other_bad_rules():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import ChordRules, generate_music
    with pytest.raises(ValueError, match="min_notes"):
        ops.check_chord_args(min_notes=5, max_notes=4)
    with pytest.raises(ValueError, match="min_notes"):
        ops.check_chord_args(min_notes=(1, 1, 7, 1), max_notes=(14, 14, 6, 14))
    with pytest.raises(ValueError, match="min_notes"):
        generate_music(None, None, chord_rules=ChordRules(min_notes=3, max_notes=2))
    with pytest.raises(ValueError, match="chord_rules"):
        generate_music(None, None, chord_rules=dict(min_notes=1))
    with pytest.raises(ValueError, match="return_note_counts"):
        generate_music(None, None, return_note_counts=True)


def test_node_track_must_be_uint8_n_on_the_logits_device():
    import torch
    from polyphemus_amd import ops
    logits = torch.zeros(3, 15, 230)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), torch.zeros(3, 1, dtype=torch.uint8),
                torch.zeros(3, dtype=torch.uint8, device="meta"), [0, 1, 2]):
        with pytest.raises(ValueError, match="node_track"):
            ops.check_chord_args(c_logits=logits, node_track=bad)
    ops.check_chord_args(c_logits=logits, node_track=torch.zeros(3, dtype=torch.uint8))


def test_chord_arguments_that_are_fine():
    import torch
    from polyphemus_amd import ops
    for kw in (dict(), dict(temperature=0), dict(temperature=(0, 1.5)), dict(temperature=[0.5, 0.0]), dict(temperature=np.float32(2)),
               dict(top_k=1), dict(top_k=10 ** 6), dict(top_p=1), dict(top_p=np.float32(0.5)), dict(seed=(1 << 32) - 1),
               dict(min_notes=0), dict(min_notes=14), dict(min_notes=(0, 1, 2, 14)), dict(max_notes=1, min_notes=0),
               dict(max_notes=(14, 1, 6, 14), min_notes=(1, 1, 2, 0)), dict(max_notes=np.int64(3)), dict(max_notes=[1, 2, 3, 4], min_notes=0),
               dict(allowed_pitches=ALL), dict(allowed_pitches=ALL.tolist()), dict(allowed_pitches=torch.zeros(4, 128, dtype=torch.bool))):
        ops.check_chord_args(**kw)
    t, mn, mx, words = ops.check_chord_args(temperature=(0.5, 2), min_notes=(1, 1, 2, 0), max_notes=(14, 1, 6, 14))
    assert t == (0.5, 2.0) and mn == (1, 1, 2, 0) and mx == (14, 1, 6, 14) and words == [[0xFFFFFFFF] * 4] * 4
    a = np.zeros((4, 128), bool)
    a[0, 0] = a[1, 31] = a[1, 32] = a[2, 127] = a[3, 60] = a[3, 95] = True
    words = ops.check_chord_args(allowed_pitches=a)[3]
    assert words == [[1, 0, 0, 0], [1 << 31, 1, 0, 0], [0, 0, 0, 1 << 31], [0, 1 << 28, 1 << 31, 0]]
    for k in range(4):                                            # the header's rule: bit (p & 31) of word (p >> 5)
        assert [p for p in range(128) if (words[k][p >> 5] >> (p & 31)) & 1] == list(np.flatnonzero(a[k]))


def test_pitch_mask_equals_its_numpy_expression():
    from polyphemus_amd.generate import ChordRules, pitch_mask
    p = np.arange(128)
    assert pitch_mask().dtype == np.bool_ and pitch_mask().shape == (128,) and pitch_mask().all()
    assert np.array_equal(pitch_mask(28, 60), (p >= 28) & (p <= 60))
    assert np.array_equal(pitch_mask(40, 88, (0, 2, 4, 5, 7, 9, 11)), (p >= 40) & (p <= 88) & np.isin(p % 12, [0, 2, 4, 5, 7, 9, 11]))
    assert np.array_equal(pitch_mask(pitch_classes=[0]), p % 12 == 0)
    assert np.array_equal(pitch_mask(60, 62), np.isin(p, [60, 61, 62]))
    assert not pitch_mask(61, 60).any() and not pitch_mask(pitch_classes=()).any()
    assert np.array_equal(pitch_mask(0, 127, {12, 14}), np.isin(p % 12, [0, 2]))          # classes are taken mod 12
    r = ChordRules()
    assert (r.min_notes, r.max_notes, r.allowed_pitches) == (1, 14, None)
