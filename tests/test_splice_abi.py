"""Checks of note splicing that need no GPU: pm_notes_splice is declared in include/polyphemus_hip.h ("Note splicing", behind
"Note statistics"), exported by the library and bound in the ctypes table with the header's argument list, the ABI version is
unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can stand in for device
addresses), and the Python surface (`ops.notes_splice`, `NoteBatch.windows` / `join`, `encode_song`, `vary_song`) rejects bad
arguments without a device."""
import re
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes
from test_stats_abi import _ids, _overlaps

SIG = "ppiilpipiipiplppppps"
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
NOTES, PTR, SEGS, SEG_PTR, SHIFT, OUT, OUT_PTR, TOTALS, KEEP, SCRATCH, STATUS = (0x10000000 + k * 0x100000 for k in range(11))
B, SRC_BARS, M, S, K, OUT_BARS, CAP = 3, 5, 50, 6, 4, 2, 40
GOOD = dict(notes=NOTES, track_ptr=PTR, B=B, src_bars=SRC_BARS, M=M, segments=SEGS, S=S, seg_ptr=SEG_PTR, K=K, out_bars=OUT_BARS,
            shift=SHIFT, silence_rule=1, out_notes=OUT, capacity=CAP, out_track_ptr=OUT_PTR, out_totals=TOTALS, keep=KEEP,
            scratch=SCRATCH, status=STATUS)
WORDS = dict(notes=3 * M, track_ptr=4 * B + 1, segments=4 * S, seg_ptr=K + 1, shift=K, out_notes=3 * CAP, out_track_ptr=4 * K + 1,
             out_totals=2, keep=K, scratch=24 * K, status=4)
INPUTS = ("notes", "track_ptr", "segments", "seg_ptr", "shift")


def _splice(**kw):
    return _lib.lib().pm_notes_splice(*{**GOOD, **kw}.values(), None)


def test_entry_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    assert protos.get("pm_notes_splice") == SIG, protos.get("pm_notes_splice")
    assert hasattr(L, "pm_notes_splice"), "pm_notes_splice not exported"
    assert _lib._SIGS.get("pm_notes_splice") == SIG and len(L.pm_notes_splice.argtypes) == len(SIG) and "pm_notes_splice" in _lib.EXPORTED
    src = open(HEADER).read()
    assert (src.index("------ Note statistics") < src.index("int pm_notes_select") < src.index("------ Note splicing")
            < src.index("int pm_notes_splice") < src.index("------ message aggregation"))
    section = src[src.index("------ Note splicing"):src.index("------ message aggregation")]
    m = re.search(r"#define PM_SPLICE_SCRATCH\(K, S\) \((.*)\)\n", section)
    assert m and eval(m.group(1).replace("(int64_t)", ""), {"K": K, "S": S}) == WORDS["scratch"]
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


BAD = ([dict(notes=None), dict(track_ptr=None), dict(segments=None), dict(seg_ptr=None), dict(out_notes=None), dict(out_track_ptr=None),
        dict(out_totals=None), dict(keep=None), dict(scratch=None), dict(status=None),
        dict(B=0), dict(B=-1), dict(K=0), dict(K=-2), dict(S=-1), dict(M=-1), dict(capacity=-1), dict(src_bars=0), dict(src_bars=-3),
        dict(out_bars=0), dict(out_bars=-1), dict(silence_rule=2), dict(silence_rule=-1), dict(out_bars=65), dict(out_bars=1 << 20),
        dict(M=(1 << 31) // 3 + 1), dict(M=1 << 62), dict(capacity=(1 << 31) // 3 + 1), dict(capacity=1 << 62), dict(B=1 << 29),
        dict(B=(1 << 31) - 1), dict(S=1 << 29), dict(K=(1 << 31) // 24 + 1), dict(src_bars=1 << 26), dict(out_bars=1 << 26, silence_rule=0),
        dict(notes=NOTES + 2), dict(track_ptr=PTR + 1), dict(segments=SEGS + 2), dict(seg_ptr=SEG_PTR + 3), dict(shift=SHIFT + 1),
        dict(out_notes=OUT + 1), dict(out_track_ptr=OUT_PTR + 2), dict(out_totals=TOTALS + 3), dict(keep=KEEP + 2), dict(scratch=SCRATCH + 2),
        dict(status=STATUS + 1)] + _overlaps(GOOD, WORDS, INPUTS))


@pytest.mark.parametrize("bad", BAD, ids=_ids)
def test_notes_splice_rejects_on_the_host(bad):
    assert _splice(**bad) == PM_E_INVALID


def test_what_may_be_null_still_checks_everything_else():
    """M == 0: notes may be NULL; S == 0: segments; capacity == 0: out_notes; shift always; the rest is checked as ever"""
    free = dict(M=0, notes=None, S=0, segments=None, capacity=0, out_notes=None, shift=None)
    for bad in (dict(status=None), dict(K=0), dict(keep=SCRATCH), dict(out_totals=TOTALS + 2), dict(out_bars=65), dict(seg_ptr=None)):
        assert _splice(**free, **bad) == PM_E_INVALID
        assert _splice(shift=None, **bad) == PM_E_INVALID


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import NoteBatch, WindowIndex, encode_song, vary_song
    nb = NoteBatch.from_lists([[[(0, 60, 4), (70, 61, 4)], [], [(5, 41, 2)], []]] * 2, 3, device="cpu")
    notes, ptr = nb.notes, nb.track_ptr
    segs, sp = torch.tensor([[0, 0, 0, 2], [1, 1, 0, 2]], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32)
    splice = lambda **kw: ops.notes_splice(**{**dict(notes=notes, track_ptr=ptr, src_bars=3, segments=segs, seg_ptr=sp, out_bars=2), **kw})
    for kw, name in ([(dict(notes=v), "notes") for v in (notes.numpy(), notes.long(), notes.reshape(-1), notes[:, :2])]
                     + [(dict(track_ptr=v), "track_ptr") for v in (ptr.tolist(), ptr.long(), ptr[:8], ptr[:1], ptr.view(1, -1))]
                     + [(dict(src_bars=v), "src_bars") for v in (0, -1, 2.0, True, None, 1 << 27)]
                     + [(dict(out_bars=v), "out_bars") for v in (0, -1, 2.0, True, None, 1 << 27)]
                     + [(dict(segments=v), "segments") for v in (segs.tolist(), segs.long(), segs[:, :3], segs.reshape(-1), None)]
                     + [(dict(seg_ptr=v), "seg_ptr") for v in (sp.tolist(), sp.long(), sp[:1], sp.view(1, -1), None)]
                     + [(dict(shift=v), "shift") for v in ([1, 2], torch.zeros(2), torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), 1)]
                     + [(dict(silence_rule=v), "silence_rule") for v in (1, None, "reference")]
                     + [(dict(silence_rule=True, out_bars=65), "out_bars <= 64")]
                     + [(dict(capacity=v), "capacity") for v in (-1, 2.0, True, 1 << 30)]):
        with pytest.raises(ValueError, match=name):
            splice(**kw)
    for kw in (dict(), dict(shift=torch.zeros(2, dtype=torch.int32), silence_rule=True, capacity=0), dict(out_bars=65, check=False)):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            splice(**kw)

    # NoteBatch.windows
    for kw, name in ([(dict(n_bars=v), "n_bars") for v in (0, -1, 2.0, True, None)] + [(dict(n_bars=2, stride=v), "stride") for v in (0, -1, 1.5, True, None)]
                     + [(dict(n_bars=2, filter=v), "filter") for v in ("none", True, 1)]
                     + [(dict(n_bars=2, seed=v), "seed") for v in (-1, 1.5, "1")]
                     + [(dict(n_bars=2, song_bars=v), "song_bars") for v in ([3], [3, 4], [3, -1], [3, 2.0], (1, 2, 3), "33", 3, torch.zeros(3, dtype=torch.int32),
                                                                           torch.zeros(2), torch.zeros(1, 2, dtype=torch.int64))]
                     + [(dict(n_bars=4), "no window"), (dict(n_bars=2, song_bars=[1, 0]), "no window")]
                     + [(dict(n_bars=2, transpose=v), "transpose") for v in (1.5, True, "up", 128, -128, [1] * 4, torch.zeros(4), torch.zeros(3, dtype=torch.int32),
                                                                           torch.zeros(4, 1, dtype=torch.int64))]
                     + [(dict(n_bars=2, song_bars=[3, 2], transpose=torch.zeros(4, dtype=torch.int32)), "K = 3")]):
        with pytest.raises(ValueError, match=name):
            nb.windows(**kw)
    big = NoteBatch(notes, ptr, nb.totals, 70)
    with pytest.raises(ValueError, match="n_bars <= 64"):
        big.windows(65, filter="reference")
    with pytest.raises(ValueError, match="notes"):
        NoteBatch(notes.long(), ptr, nb.totals, 3).windows(2)
    for kw in (dict(n_bars=2), dict(n_bars=1, stride=2, song_bars=[3, 1], filter="reference", transpose="random", seed=4),
               dict(n_bars=3, transpose=torch.zeros(2, dtype=torch.int64)), dict(n_bars=2, song_bars=torch.tensor([3, 2]), transpose=-5)):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            nb.windows(**kw)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        big.windows(65)

    # NoteBatch.join
    for bad in (0, -1, 4, 1.0, True, "1"):
        with pytest.raises(ValueError, match="hop_bars"):
            nb.join([[0, 1]], hop_bars=bad)
    for bad in ([], [[]], [0, 1], [[0, 1], [1]], [[0.5]], [[True]], "01", None, 3, torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2),
                torch.zeros(0, 2, dtype=torch.int32), torch.zeros(1, 1, 1, dtype=torch.int32), [[1 << 31]], np.zeros((1, 2), np.int64)):
        with pytest.raises(ValueError, match="index"):
            nb.join(bad)
    with pytest.raises(ValueError, match="too many"):
        nb.join(torch.zeros(1, 1, dtype=torch.int32).expand(1, 1 << 26))
    for index, kw in (([[0, 1]], {}), ([[1], [-1]], dict(hop_bars=1)), (torch.tensor([[0, -1, 1]]), dict(check=False)),
                      (torch.tensor([[1, 0]], dtype=torch.int32), dict(hop_bars=3))):
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            nb.join(index, **kw)
    assert [f.name for f in WindowIndex.__dataclass_fields__.values()] == ["song", "start", "shift"]

    # encode_song / vary_song: before the model is touched
    vae = types.SimpleNamespace(cfg=dict(n_bars=2))
    for bad in (None, nb.tolist(), notes):
        with pytest.raises(ValueError, match="song must be a NoteBatch"):
            encode_song(vae, bad)
        with pytest.raises(ValueError, match="song must be a NoteBatch"):
            vary_song(vae, bad)
    for bad in (0, -2, 2.5, None):
        with pytest.raises(ValueError, match="n_bars"):
            encode_song(vae, NoteBatch(notes, ptr, nb.totals, bad))
    for bad in (-1, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="strength"):
            vary_song(vae, nb, strength=bad)
    for kw, name in ((dict(return_tokens=True), "return_tokens"), (dict(return_z=False), "return_z")):
        with pytest.raises(ValueError, match=name):
            vary_song(vae, nb, **kw)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        encode_song(vae, nb)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        vary_song(vae, nb, strength=0)
