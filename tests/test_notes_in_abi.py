"""Checks of "notes in" that need no GPU: pm_tokens_from_notes is declared in include/polyphemus_hip.h ("Notes in", behind "Note
events"), exported by the library and bound in the ctypes table with the header's argument list, the ABI version is
unchanged, every argument check answers PM_E_INVALID on the host before any launch (so host integers can stand in for device
addresses), the Python surface rejects bad arguments without a device, and the numpy restatement the GPU tests compare with
(tests/notes_in_util.py) gives back the golden cases' own structure and tokens from the notes `notes_ref` reads out of them."""
import os
import re
import types

import numpy as np
import pytest
import torch

from polyphemus_amd import _lib
from notes_in_util import as_batch, check_ref, end_clamped, notes_ref, tokens_ref
from notes_util import CASES, GOLDEN
from test_abi import HEADER, header_prototypes

NAME, SIG = "pm_tokens_from_notes", "ppiilpplpps"
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
NOTES, TRACK_PTR, S, TOKENS, SCRATCH, STATUS = (0x10000000 + k * 0x100000 for k in range(6))
B, NB, M, CAP = 3, 2, 40, 46
G = B * NB
N_SCRATCH = 3 * G + 1 + 12 * B
GOOD = dict(notes=NOTES, track_ptr=TRACK_PTR, B=B, n_bars=NB, M=M, s_tensor=S, tokens=TOKENS, capacity=CAP, scratch=SCRATCH,
            status=STATUS)


def _call(**kw):
    return _lib.lib().pm_tokens_from_notes(*{**GOOD, **kw}.values(), None)


def test_entry_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    assert protos.get(NAME) == SIG, protos.get(NAME)
    assert hasattr(L, NAME), f"{NAME} not exported"
    assert _lib._SIGS.get(NAME) == SIG and len(getattr(L, NAME).argtypes) == len(SIG) and NAME in _lib.EXPORTED
    src = open(HEADER).read()
    assert src.index("Note events") < src.index("Notes in") and "preprocess.py:118-157" in src and "data.py:148-153" in src
    assert re.search(r"#define PM_NOTES_IN_SCRATCH\(B, n_bars\) \(3 \* \(int64_t\)\(B\) \* \(n_bars\) \+ 1 \+ 12 \* \(int64_t\)\(B\)\)", src)
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


BAD = [dict(notes=None), dict(track_ptr=None), dict(s_tensor=None), dict(tokens=None), dict(scratch=None), dict(status=None),
       dict(B=0), dict(B=-3), dict(n_bars=0), dict(n_bars=-2), dict(M=-1), dict(M=-(1 << 40)), dict(capacity=-1),
       # sizes beyond 32 bits: 128 G, 3 M, 32 capacity
       dict(B=1 << 24, n_bars=1), dict(B=1 << 12, n_bars=1 << 12), dict(M=1 << 30), dict(M=1 << 40), dict(capacity=1 << 26),
       dict(capacity=1 << 62),
       # misaligned: 4 bytes for every buffer, 16 for the tokens
       dict(notes=NOTES + 2), dict(track_ptr=TRACK_PTR + 1), dict(s_tensor=S + 2), dict(scratch=SCRATCH + 3), dict(status=STATUS + 2),
       dict(tokens=TOKENS + 4), dict(tokens=TOKENS + 8),
       # overlapping: the same buffer, and ranges that share their last / first element
       dict(s_tensor=NOTES), dict(tokens=NOTES), dict(scratch=TRACK_PTR), dict(status=TRACK_PTR + 4 * 4 * B), dict(status=NOTES + 4 * (3 * M - 1)),
       dict(tokens=S), dict(scratch=S + 4 * (128 * G - 1)), dict(status=S), dict(scratch=TOKENS), dict(status=TOKENS + 4 * (32 * CAP - 1)),
       dict(status=SCRATCH), dict(status=SCRATCH + 4 * (N_SCRATCH - 1)), dict(scratch=STATUS + 4 * 4), dict(s_tensor=TOKENS + 16 * (8 * CAP - 1))]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_tokens_from_notes_rejects_on_the_host(bad):
    assert _call(**bad) == PM_E_INVALID


def test_no_rows_and_no_capacity_still_check_everything_else():
    """M == 0: notes may be NULL; capacity == 0: tokens may be NULL; the other arguments are checked as ever"""
    for kw in (dict(M=0, notes=None), dict(capacity=0, tokens=None), dict(M=0, notes=None, capacity=0, tokens=None)):
        assert _call(**kw, status=None) == PM_E_INVALID
        assert _call(**kw, B=0) == PM_E_INVALID
        assert _call(**kw, status=SCRATCH) == PM_E_INVALID
        assert _call(**kw, s_tensor=S + 2) == PM_E_INVALID


def test_python_surface_rejects_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import NoteBatch, StructureRules, encode_notes, vary_notes
    from polyphemus_amd.graphs import device_batch_from_notes
    notes, ptr = torch.zeros(5, 3, dtype=torch.int32), torch.tensor([0, 1, 2, 3, 5], dtype=torch.int32)
    for fn in (ops.tokens_from_notes, device_batch_from_notes):
        for bad in (notes.long(), notes.float(), notes[:, :2], notes.reshape(-1), notes.reshape(1, 5, 3), [[0, 1, 2]]):
            with pytest.raises(ValueError, match="notes"):
                fn(bad, ptr, 2)
        for bad in (ptr.long(), ptr[:4], ptr[:1], ptr.reshape(1, 5), torch.zeros(6, dtype=torch.int32), [0, 1, 2, 3, 5]):
            with pytest.raises(ValueError, match="track_ptr"):
                fn(notes, bad, 2)
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="n_bars"):
                fn(notes, ptr, bad)
        with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
            fn(notes, ptr, 2)
    # NoteBatch.from_lists: everything is checked before the device is touched (device="meta" would fail otherwise)
    ok = [[[(0, 60, 4)], [], [(63, 40, 1), (5, 41, 2)], []]]
    for pieces, nb, name in (([], 2, "pieces"), ("x", 2, "pieces"), ([[[], [], []]], 2, "four lists"), ([[[], [], [], [], []]], 2, "four lists"),
                             ([[[], [], [], 3]], 2, "four lists"), ([[[(0, 60)], [], [], []]], 2, "three ints"),
                             ([[[(0, 60, 4.0)], [], [], []]], 2, "three ints"), ([[[(0, True, 4)], [], [], []]], 2, "three ints"),
                             ([[[], [5], [], []]], 2, "three ints"), ([[[(0, 1 << 31, 4)], [], [], []]], 2, "three ints"),
                             ([[[], [], [], [(64, 60, 4)]]], 2, "time 64"), ([[[(-1, 60, 4)], [], [], []]], 2, "time -1"),
                             (ok, 1, "time 63"), (ok, 0, "n_bars"), (ok, 2.5, "n_bars")):
        with pytest.raises(ValueError, match=name):
            NoteBatch.from_lists(pieces, nb, device="no-such-device")
    nb = NoteBatch.from_lists(ok, 2, device="cpu")
    assert nb.n_bars == 2 and nb.resolution == 8 and nb.tolist() == [[[(0, 60, 4)], [], [(5, 41, 2), (63, 40, 1)], []]]
    assert nb.track_ptr.tolist() == [0, 1, 1, 3, 3] and nb.totals.tolist() == [3, 3] and nb.notes.dtype == torch.int32
    # equal times keep their list order (a stable sort), and from_lists(tolist()) is the identity
    chord = [[[(3, 9, 1), (0, 7, 1), (3, 2, 1), (3, 5, 1), (0, 1, 1)], [], [], []], [[], [], [], []]]
    nb = NoteBatch.from_lists(chord, 1, device="cpu", resolution=4)
    assert nb.tolist()[0][0] == [(0, 7, 1), (0, 1, 1), (3, 9, 1), (3, 2, 1), (3, 5, 1)] and nb.totals.tolist() == [5, 2] and nb.resolution == 4
    again = NoteBatch.from_lists(nb.tolist(), 1, device="cpu")
    assert torch.equal(again.notes, nb.notes) and torch.equal(again.track_ptr, nb.track_ptr)
    notes_np, ptr_np = as_batch(chord)
    assert np.array_equal(nb.notes.numpy(), notes_np) and np.array_equal(nb.track_ptr.numpy(), ptr_np)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        nb.to_graph()
    # encode_notes / vary_notes: before the model is touched
    vae = types.SimpleNamespace(cfg={"n_bars": 3})
    for fn in (encode_notes, vary_notes):
        with pytest.raises(ValueError, match="NoteBatch"):
            fn(vae, (nb.notes, nb.track_ptr))
        with pytest.raises(ValueError, match="n_bars = 1"):
            fn(vae, nb)
    for kw, name in ((dict(strength=-0.5), "strength"), (dict(strength=float("inf")), "strength"), (dict(strength=float("nan")), "strength"),
                     (dict(strength="1"), "strength"), (dict(seed=-1), "seed"), (dict(seed=1 << 32), "seed"), (dict(seed=1.5), "seed"),
                     (dict(s_cond=3), "s_cond"), (dict(s_tensor_cond=3), "s_tensor_cond"),
                     (dict(keep_structure=True, structure_rules=StructureRules()), "structure_rules draws the structure itself")):
        with pytest.raises(ValueError, match=name):
            vary_notes(None, None, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_gives_the_golden_cases_back(name):
    """the golden batch -> its notes (`notes_ref`, which tests/test_notes_golden.py ties to notes recorded from the reference)
    -> the restatement: the reference's own structure and tokens, but for the durations the reader cut at the piece's end"""
    n_bars = CASES[name][1]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    tokens, s = z["in/tokens"].astype(np.int32), z["in/s_tensor"]
    notes, ptr = notes_ref(tokens[:, 1:], s.reshape(-1, n_bars, 4, 32))
    assert check_ref(notes, ptr, n_bars) == (0, 0, 0)
    s2, tokens2, dropped = tokens_ref(notes, ptr, n_bars)
    want = end_clamped(tokens, s, n_bars)
    assert dropped == 0 and s2.dtype == np.float32 and np.array_equal(s2, s.astype(np.float32))
    assert tokens2.dtype == np.int32 and np.array_equal(tokens2, want)
    assert np.array_equal(tokens2[..., 0], tokens[..., 0])
    changed = tokens2[..., 1] != tokens[..., 1]
    assert changed.any() and (tokens2[..., 1][changed] < tokens[..., 1][changed]).all()
