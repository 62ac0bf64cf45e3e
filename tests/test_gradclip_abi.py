"""C-ABI checks of the gradient clipping by the global norm that need no GPU: its entries are declared in
include/polyphemus_hip.h, exported by the library and bound in the ctypes table with the header's argument list; the
PM_CLIP_* layout equals the constants of `ops`; the trainer rejects a bad `max_grad_norm` before it touches the model."""
import re

import pytest

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes

ENTRIES = {"pm_grad_sumsq": "plps", "pm_grad_nonfinite_check_sumsq": "plpppfffips", "pm_grad_clip_finish": "pffps",
           "pm_adam_step_clipped": "pppplffffipps"}


def test_clip_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)
    # the entries they stand beside keep their argument lists
    assert protos["pm_grad_nonfinite_check"] == "plpppfffis" and protos["pm_adam_step_guarded"] == "pppplffffps"
    assert protos["pm_adam_step"] == "pppplffffifs"


def test_clip_abi_version_and_block_layout():
    src = open(HEADER).read()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.lib().pm_abi_version()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(PM_CLIP_\w+)\s*=\s*(\d+)", src))
    from polyphemus_amd import ops
    assert set(enum) == {"PM_CLIP_NORM", "PM_CLIP_COEF", "PM_CLIP_GSCALE", "PM_CLIP_SUMSQ", "PM_CLIP_PARTIALS_AT",
                         "PM_CLIP_PARTIALS", "PM_CLIP_WORDS"}
    for k in ("NORM", "COEF", "GSCALE", "SUMSQ", "PARTIALS_AT", "PARTIALS", "WORDS"):
        assert enum[f"PM_CLIP_{k}"] == getattr(ops, f"CLIP_{k}"), k
    assert enum["PM_CLIP_WORDS"] == enum["PM_CLIP_PARTIALS_AT"] + enum["PM_CLIP_PARTIALS"]
    assert len({enum[f"PM_CLIP_{k}"] for k in ("NORM", "COEF", "GSCALE", "SUMSQ")}) == 4
    assert max(enum[f"PM_CLIP_{k}"] for k in ("NORM", "COEF", "GSCALE", "SUMSQ")) < enum["PM_CLIP_PARTIALS_AT"]
    assert int(re.search(r"\bPM_OVF_WORDS\s*=\s*(\d+)", src).group(1)) == 8 == ops.OVF_WORDS


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, 1e-50, float("nan"), "1", float("-inf"), True])
def test_trainer_rejects_bad_max_grad_norm(bad):
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, max_grad_norm=bad)


@pytest.mark.parametrize("bad", [0, -3, 1.5, "8"])
def test_trainer_rejects_bad_grad_norm_capacity(bad):
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="grad_norm_capacity"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, max_grad_norm=1.0, grad_norm_capacity=bad)
