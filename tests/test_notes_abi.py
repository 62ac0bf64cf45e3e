"""Checks of the note events that need no GPU: pm_notes_from_tokens is declared in include/polyphemus_hip.h ("Note events"),
exported by the library and bound in the ctypes table with the header's argument list, the ABI version is unchanged, every
argument check answers PM_E_INVALID on the host before any launch (so host integers can stand in for device addresses), and
`ops.notes_from_tokens`, `generate_notes` and `NoteBatch` reject bad arguments without a device."""
import re

import pytest
import torch

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes

NAME, SIG = "pm_notes_from_tokens", "ppiilppppplpps"
PM_E_INVALID = -1
# fake device addresses, 16-byte aligned and 1 MiB apart
TOKENS, S, SEG_COUNT, SEG_PTR, BARS, PTR, NOTES, TRACK_PTR, TOTALS = (0x10000000 + k * 0x100000 for k in range(9))
G, NB, N = 6, 3, 7
GOOD = dict(tokens=TOKENS, s_tensor=S, G=G, n_bars=NB, N=N, seg_count=SEG_COUNT, seg_ptr=SEG_PTR, bar_nodes=BARS, node_ptr=PTR,
            notes=NOTES, capacity=15 * N, track_ptr=TRACK_PTR, totals=TOTALS)


def _notes(**kw):
    return _lib.lib().pm_notes_from_tokens(*{**GOOD, **kw}.values(), None)


def test_notes_entry_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    assert protos.get(NAME) == SIG, protos.get(NAME)
    assert hasattr(L, NAME), f"{NAME} not exported"
    assert _lib._SIGS.get(NAME) == SIG and len(getattr(L, NAME).argtypes) == len(SIG) and NAME in _lib.EXPORTED
    src = open(HEADER).read()
    assert "Note events" in src and src.index("sampled generation") < src.index("Note events") and "utils.py:83-124" in src
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == L.pm_abi_version()


BAD = [dict(capacity=15 * N - 1), dict(capacity=0), dict(capacity=-1), dict(G=7), dict(G=4, n_bars=3), dict(n_bars=0), dict(n_bars=-3),
       dict(G=0), dict(G=-6), dict(N=-1), dict(N=-(1 << 40), capacity=0), dict(N=1 << 40, capacity=1 << 62), dict(G=3 << 28),
       dict(tokens=None), dict(s_tensor=None), dict(seg_count=None), dict(seg_ptr=None), dict(bar_nodes=None), dict(node_ptr=None),
       dict(notes=None), dict(track_ptr=None), dict(totals=None), dict(tokens=TOKENS + 4),
       # aliasing scratch and outputs: the same buffer, and ranges that share their last / first element
       dict(node_ptr=BARS), dict(seg_ptr=SEG_COUNT), dict(seg_ptr=SEG_COUNT + 4 * (4 * G - 1)), dict(seg_count=SEG_PTR + 4 * 4 * G),
       dict(bar_nodes=PTR + 4 * G), dict(node_ptr=SEG_PTR), dict(track_ptr=SEG_PTR), dict(totals=TRACK_PTR + 4 * (4 * G // NB)),
       dict(totals=NOTES + 4 * (3 * 15 * N - 1)), dict(notes=SEG_COUNT), dict(track_ptr=BARS), dict(totals=PTR)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_notes_from_tokens_rejects_on_the_host(bad):
    assert _notes(**bad) == PM_E_INVALID


def test_no_nodes_still_checks_everything_else():
    """N == 0: tokens and notes may be NULL; the other arguments are checked as ever"""
    assert _notes(N=0, capacity=0, tokens=None, notes=None, totals=None) == PM_E_INVALID
    assert _notes(N=0, capacity=0, tokens=None, notes=None, node_ptr=BARS) == PM_E_INVALID
    assert _notes(N=0, capacity=0, tokens=None, notes=None, G=7) == PM_E_INVALID


def test_ops_and_generate_notes_reject_bad_arguments_without_a_device():
    from polyphemus_amd import ops
    from polyphemus_amd.generate import ChordRules, NoteBatch, generate_notes
    tok, s = torch.zeros(3, 15, 2, dtype=torch.int32), torch.zeros(1, 2, 4, 32)
    for bad_tok in (tok.long(), tok.float(), tok[:, :14], tok.reshape(3, 30), tok[..., :1], [[0]]):
        with pytest.raises(ValueError, match="tokens"):
            ops.notes_from_tokens(bad_tok, s)
    for bad_s in (s[0], s[..., :31], torch.zeros(1, 2, 3, 32), torch.zeros(0, 2, 4, 32), torch.zeros(2, 0, 4, 32)):
        with pytest.raises(ValueError, match="s_tensor"):
            ops.notes_from_tokens(tok, bad_s)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        ops.notes_from_tokens(tok, s)
    # generate_notes: generate_music's checks, before the model (None here) is touched
    for kw, name in ((dict(temperature=-1.0), "temperature"), (dict(top_k=0), "top_k"), (dict(top_p=2.0), "top_p"), (dict(seed=-1), "seed"),
                     (dict(chord_rules=3), "chord_rules"), (dict(chord_rules=ChordRules(min_notes=3, max_notes=2)), "min_notes"),
                     (dict(structure_rules=3), "structure_rules")):
        with pytest.raises(ValueError, match=name):
            generate_notes(None, None, **kw)
    assert NoteBatch(None, None, None, 2).resolution == 8


def test_to_muspy_without_muspy_raises_a_clear_import_error(monkeypatch):
    import sys
    from polyphemus_amd.generate import NoteBatch
    monkeypatch.setitem(sys.modules, "muspy", None)              # `import muspy` now raises ImportError, installed or not
    with pytest.raises(ImportError, match="muspy"):
        NoteBatch(None, None, None, 2).to_muspy(0, {})
