"""Training accuracies, the checks that need no GPU: the new C entries are declared in include/polyphemus_hip.h, exported by
the library and bound with the header's argument lists; the ABI version stays 9; the trainer rejects a bad option; the
counts -> accuracies arithmetic."""
import math
import re

import pytest

from polyphemus_amd import _lib, ops
from test_abi import HEADER, header_prototypes

ENTRIES = {"pm_vae_step_set_metrics": "pp",
           "pm_unembed_ce_metrics": "pppppppppiiiiifppppppppppps",
           "pm_unembed_ce_rows_metrics": "pppppppppiiiiifppppppppppppps",
           "pm_content_accuracy_slots": "pppiipps",
           "pm_train_metric_counts": "pppiipplps"}


def test_train_metrics_entries_declared_exported_and_bound():
    protos = header_prototypes()
    L = _lib.lib()
    for name, sig in ENTRIES.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert hasattr(L, name), f"{name} not exported"
        assert _lib._SIGS.get(name) == sig, (name, _lib._SIGS.get(name))
        assert len(getattr(L, name).argtypes) == len(sig)


def test_metrics_entries_extend_the_existing_ones():
    # the kernel-level entries are the existing argument lists plus (is_drum, verdict, counts)
    assert ENTRIES["pm_unembed_ce_metrics"] == _lib._SIGS["pm_unembed_ce"][:-1] + "ppps"
    assert ENTRIES["pm_unembed_ce_rows_metrics"] == _lib._SIGS["pm_unembed_ce_rows"][:-1] + "ppps"


def test_abi_version_still_9():
    src = open(HEADER).read()
    assert int(re.search(r"#define PM_ABI_VERSION (\d+)", src).group(1)) == 9 == _lib.ABI_VERSION == _lib.lib().pm_abi_version()


@pytest.mark.parametrize("bad", ["yes", 1, None, 0.0])
def test_trainer_rejects_bad_train_metrics(bad):
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="train_metrics"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, train_metrics=bad)


def test_trainer_rejects_bad_capacity():
    from polyphemus_amd.trainer import HipTrainer
    with pytest.raises(ValueError, match="metrics_capacity"):
        HipTrainer.__init__(object.__new__(HipTrainer), None, train_metrics=True, metrics_capacity=0)


def test_accuracies_from_counts_ratios():
    c = [30, 40, 5, 8, 20, 40, 12, 0, 500, 60, 80, 90, 512, 0, 0, 0]
    a = ops.accuracies_from_counts(c)
    assert list(a) == list(ops.ACCURACY_KEYS)
    prec, rec = 60 / 80, 60 / 90
    want = {"note": 12 / 40, "pitch": 30 / 40, "pitch_drums": 5 / 8, "pitch_non_drums": 25 / 32, "dur": 20 / 40,
            "s_acc": 500 / 512, "s_precision": prec, "s_recall": rec, "s_f1": 2 * rec * prec / (rec + prec)}
    for k, v in want.items():
        assert a[k] == pytest.approx(v, rel=1e-15), k


def test_accuracies_from_counts_nan_on_zero_denominators():
    # no drum tokens: pitch_drums is 0 / 0; no predicted positives: precision (and F1) NaN
    a = ops.accuracies_from_counts([3, 4, 0, 0, 2, 4, 1, 0, 7, 0, 0, 5, 8, 0, 0, 0])
    assert math.isnan(a["pitch_drums"]) and math.isnan(a["s_precision"]) and math.isnan(a["s_f1"])
    assert a["pitch_non_drums"] == 3 / 4 and a["pitch"] == 3 / 4 and a["s_recall"] == 0.0 and a["s_acc"] == 7 / 8
    b = ops.accuracies_from_counts([0] * 16)
    assert all(math.isnan(b[k]) for k in ("note", "pitch", "pitch_drums", "pitch_non_drums", "dur", "s_precision",
                                          "s_recall", "s_f1"))
    assert b["s_acc"] == 0.0
