"""C-ABI checks of the guarded optimizer step that need no GPU: its entries are declared in include/polyphemus_hip.h,
exported by the library and bound in the ctypes table with the header's argument list."""
import re

from polyphemus_amd import _lib
from test_abi import HEADER, header_prototypes

ENTRIES = {"pm_h2_clamp_init": "", "pm_overflow_snapshot": "ps", "pm_overflow_poison": "pps",
           "pm_grad_nonfinite_check": "plpppfffis", "pm_adam_step_guarded": "pppplffffps", "pm_adam_bias_scalars": "plfffps"}


def test_guarded_step_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)


def test_guarded_step_abi_version_and_status_layout():
    src = open(HEADER).read()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.lib().pm_abi_version()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(PM_OVF_\w+)\s*=\s*(\d+)", src))
    from polyphemus_amd import ops
    assert enum["PM_OVF_WORDS"] == ops.OVF_WORDS
    for k in ("PENDING", "LAST", "SNAP", "N_NONFINITE", "N_SATURATED", "STEP_SIZE", "INV_BC2", "TICKET"):
        assert enum[f"PM_OVF_{k}"] == getattr(ops, f"OVF_{k}"), k
    assert (enum["PM_OVF_NONFINITE_BIT"], enum["PM_OVF_SATURATED_BIT"]) == (ops.OVF_NONFINITE_BIT, ops.OVF_SATURATED_BIT)


def test_trainer_rejects_unknown_overflow_policy():
    import pytest
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="overflow"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, overflow="clip")
